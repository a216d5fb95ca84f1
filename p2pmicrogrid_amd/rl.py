"""Learners (mirrors microgrid/rl.py:36-132 for the tabular actor).

``QActor`` keeps the reference's constructor, attributes and methods.  Its table lives in HBM:
inside a ``CommunityMicrogrid`` it is the agent's slot of the community's device tables
(the episode kernel reads and updates it); a standalone actor owns a private one-agent device
context.  ``q_table`` / ``set_qtable`` copy to / from the reference layout
(n_time, n_temp, n_balance, n_p2p, n_actions) float64, and ``load_from_file`` /
``save_to_file`` read / write the reference's ``.npy`` checkpoints (rl.py:83-87);
``save_sparse`` / ``load_sparse`` the sparse ``.npz`` form (``sparse_table`` states the format).
Per-call ``select_action`` / ``greedy_action`` / ``train`` run on the device (p2pmg_q_calls);
the exploration draws use the global np.random exactly as rl.py:101-111 does.
"""
from __future__ import annotations

import os
from abc import ABC, abstractmethod
from typing import Optional, Tuple

import numpy as np

from . import setup

MODELS_DIR = os.environ.get("P2PMG_MODELS_DIR", "..")  # the reference uses ../models_{implementation}/


def _as_obs(state) -> np.ndarray:
    x = state.numpy() if hasattr(state, "numpy") else state
    return np.asarray(x, dtype=np.float32).reshape(-1, 4)


def table_digest(q_table: np.ndarray) -> Tuple[np.ndarray, dict]:
    """include/p2pmg.h's table digests of one table [..., n_actions] on the host, for an actor whose table
    is not on a device: (packed greedy policy u8 [...], 255 = unvisited row; the p2pmg_table_stats
    fields).  A row is visited iff any entry != 0; its greedy action is the first maximum (rl.py:116)."""
    q = np.asarray(q_table)
    na = q.shape[-1]
    visited = (q != 0).any(axis=-1)
    greedy = np.zeros(q.shape[:-1], np.uint8)
    best = q[..., 0]
    for k in range(1, na):  # the device's scan: strictly greater replaces
        better = q[..., k] > best
        best = np.where(better, q[..., k], best)
        greedy[better] = k
    lo, hi = np.float64(q.min()), np.float64(q.max())
    stats = {"visited": np.int64(visited.sum()), "q_min": lo + 0.0, "q_max": hi + 0.0,
             "abs_max": np.float64(max(-lo, hi)) + 0.0,
             "greedy": np.array([(visited & (greedy == k)).sum() for k in range(na)], np.int64)}
    return np.where(visited, greedy, np.uint8(255)).astype(np.uint8), stats


SPARSE_KEYS = ("shape", "offsets", "rows", "values")


def _bits(x: np.ndarray) -> np.ndarray:
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def sparse_table(q_table: np.ndarray) -> dict:
    """The sparse form of include/p2pmg.h on the host: one table (n_time, n_temp, n_balance, n_p2p,
    n_actions), or tables [count, ...] (six axes), f64 or f32 (anything else is taken as f64) ->
    {"shape": the table shape int64 [5], "offsets": int64 [count + 1], "rows": int32 [total], "values":
    [total, n_actions]}.  A row is stored iff one of its entries has a non-zero BIT pattern (-0.0
    counts); rows holds the state indices of the stored rows, table after table (table k's are
    rows[offsets[k]:offsets[k + 1]]), ascending inside each table; values their entries, same order."""
    q = np.asarray(q_table)
    if q.dtype not in (np.float64, np.float32):
        q = q.astype(np.float64)
    if q.ndim not in (5, 6):
        raise ValueError(f"one table (5 axes) or [count, ...] tables (6 axes), got shape {q.shape}")
    shape = q.shape[-5:]
    flat = np.ascontiguousarray(q).reshape(-1, int(np.prod(shape[:-1])), shape[-1])
    if flat.shape[1] > 2 ** 31 - 1:
        raise ValueError("row indices are int32: at most 2^31 - 1 states")
    table, row = np.nonzero((_bits(flat) != 0).any(axis=-1))  # row-major: by table, then ascending row
    offsets = np.zeros(flat.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(table, minlength=flat.shape[0]), out=offsets[1:])
    return {"shape": np.asarray(shape, np.int64), "offsets": offsets, "rows": row.astype(np.int32),
            "values": flat[table, row]}


def check_sparse(sparse, shape=None) -> Tuple[tuple, np.ndarray, np.ndarray, np.ndarray]:
    """(shape, offsets int64, rows int32, values f64 | f32) of a sparse form, or ValueError where it is
    none: keys, array shapes, offsets from 0 to len(rows) without a step back or one above n_states, every
    index in [0, n_states) and strictly ascending inside its table; shape: the table shape it must have."""
    missing = [k for k in SPARSE_KEYS if k not in sparse]
    if missing:
        raise ValueError(f"not a sparse table form: no {missing}")
    shp = tuple(int(x) for x in np.asarray(sparse["shape"]).reshape(-1))
    if len(shp) != 5 or min(shp) < 1:
        raise ValueError(f"sparse form: bad table shape {shp}")
    if shape is not None and shp != tuple(shape):
        raise ValueError(f"sparse form holds tables of shape {shp}, not {tuple(shape)}")
    offsets = np.ascontiguousarray(sparse["offsets"], np.int64).reshape(-1)
    rows = np.ascontiguousarray(sparse["rows"], np.int32).reshape(-1)
    values = np.asarray(sparse["values"])
    values = np.ascontiguousarray(values, values.dtype if values.dtype in (np.float64, np.float32) else np.float64)
    n_states = int(np.prod(shp[:-1]))
    steps = np.diff(offsets)
    if offsets.size < 1 or offsets[0] != 0 or offsets[-1] != rows.size or (steps < 0).any() or (steps > n_states).any():
        raise ValueError("sparse form: offsets do not run from 0 to len(rows) in steps within [0, n_states]")
    if values.shape != (rows.size, shp[-1]):
        raise ValueError(f"sparse form: values {values.shape} for {rows.size} rows of {shp[-1]} actions")
    if rows.size and (rows.min() < 0 or rows.max() >= n_states):
        raise ValueError("sparse form: row index outside [0, n_states)")
    starts = np.zeros(rows.size, bool)
    starts[offsets[:-1][steps > 0]] = True  # the first index of a table need not exceed the one before it
    if rows.size and (np.diff(rows.astype(np.int64)) <= 0)[~starts[1:]].any():
        raise ValueError("sparse form: row indices not strictly ascending inside a table")
    return shp, offsets, rows, values


def dense_table(sparse) -> np.ndarray:
    """[count, *shape] in the dtype of ``values``: zeros (+0.0), then the stored rows written.
    ``dense_table(sparse_table(q))`` has q's bytes, except that it always has the leading count axis."""
    shp, offsets, rows, values = check_sparse(sparse)
    count = offsets.size - 1
    out = np.zeros((count, int(np.prod(shp[:-1])), shp[-1]), values.dtype)
    out[np.repeat(np.arange(count), np.diff(offsets)), rows] = values
    return out.reshape(count, *shp)


def save_sparse_file(path: str, sparse) -> str:
    """One uncompressed .npz with exactly the four keys of the sparse form; returns the path written."""
    shp, offsets, rows, values = check_sparse(sparse)
    path = path if path.endswith(".npz") else path + ".npz"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    np.savez(path, shape=np.asarray(shp, np.int64), offsets=offsets, rows=rows, values=values)
    return path


def load_sparse_file(path: str, shape=None) -> dict:
    """The sparse form a file holds (allow_pickle=False), checked; ValueError where it is none or where its
    tables are not of ``shape``."""
    with np.load(path if path.endswith(".npz") else path + ".npz", allow_pickle=False) as f:
        shp, offsets, rows, values = check_sparse({k: f[k] for k in f.files}, shape)
    return {"shape": np.asarray(shp, np.int64), "offsets": offsets, "rows": rows, "values": values}


class ActorInterface(ABC):
    @abstractmethod
    def __call__(self, state, *args, **kwargs): ...

    @abstractmethod
    def select_action(self, state): ...

    @abstractmethod
    def greedy_action(self, state): ...

    @abstractmethod
    def load_from_file(self, setting: str, implementation: str) -> None: ...

    @abstractmethod
    def save_to_file(self, setting: str, implementation: str) -> None: ...

    @abstractmethod
    def decay_exploration(self) -> None: ...


class QActor(ActorInterface):

    def __init__(self, num_time_states: int, num_temperature_states: int, num_balance_states: int,
                 num_p2p_states: int, num_actions: int = 3, gamma: float = 0.9,
                 alpha: float = 1e-5, epsilon: float = 1, decay: float = 0.9) -> None:
        self._time_states = num_time_states
        self._temp_states = num_temperature_states
        self._balance_states = num_balance_states
        self._p2p_states = num_p2p_states
        self._num_actions = num_actions
        self._epsilon = epsilon
        self._decay = decay
        self._gamma = gamma
        self._alpha = alpha
        self._shape = (num_time_states, num_temperature_states, num_balance_states, num_p2p_states, num_actions)
        self._host_table: Optional[np.ndarray] = None  # pending table while unbound (None = zeros)
        self._engine = None
        self._slot = 0

    # ------------------------------------------------------------ device binding
    def bind(self, engine, slot: int) -> None:
        """Attach to agent ``slot`` of a DeviceCommunityBatch (uploads any pending table)."""
        if engine.q_shape != self._shape:
            raise ValueError(f"QActor table shape {self._shape} != device {engine.q_shape}")
        table = self._host_table if self._engine is None else self.q_table
        self._engine, self._slot = engine, slot
        self._host_table = None
        # this actor's own alpha and gamma (rl.py:58-71) into its slot of the engine's per-agent arrays
        # (a slot is an agent where every agent has its table; shared tables keep the engine's values)
        if engine.n_tables == engine.A:
            cur = engine.get_learning()
            a, g = cur["alpha"].reshape(-1), cur["gamma"].reshape(-1)
            if (a[slot], g[slot]) != (self._alpha, self._gamma):
                a[slot], g[slot] = self._alpha, self._gamma
                engine.set_learning(alpha=a, gamma=g, penalty_weight=cur["penalty_weight"])
        if table is not None:
            engine.set_q(np.asarray(table)[None], first=slot)

    def _device(self):
        if self._engine is None:
            from .engine import DeviceCommunityBatch
            nt, nT, nb, np_, na = self._shape
            eng = DeviceCommunityBatch(1, 1, 0, 1, q_dtype=setup.q_dtype, device=setup.device,
                                       alpha=self._alpha, gamma=self._gamma, n_time_states=nt,
                                       n_temp_states=nT, n_balance_states=nb, n_p2p_states=np_)
            self.bind(eng, 0)
        return self._engine, self._slot

    # ------------------------------------------------------------ table access (rl.py:76-87)
    @property
    def q_table(self) -> np.ndarray:
        if self._engine is None:
            return np.zeros(self._shape) if self._host_table is None else self._host_table
        return self._engine.get_q(first=self._slot, count=1)[0]

    def set_qtable(self, q_table: np.ndarray) -> None:
        q_table = np.asarray(q_table)
        if q_table.shape != self._shape:
            raise ValueError(f"q_table shape {q_table.shape} != {self._shape}")
        if self._engine is None:
            self._host_table = np.array(q_table, dtype=np.float64)
        else:
            self._engine.set_q(q_table[None], first=self._slot)

    def greedy_policy(self) -> np.ndarray:
        """u8 (n_time, n_temp, n_balance, n_p2p): every state's greedy action, 255 where the row was
        never written.  Bound: packed on the device (p2pmg_greedy_policy), 1/32 of the f64 table."""
        if self._engine is None:
            return table_digest(self.q_table)[0]
        return self._engine.greedy_policy(first=self._slot, count=1)[0]

    def policy_bytes(self) -> np.ndarray:
        """u8 [n_states]: greedy_policy() flattened in table-row order, bound or not: one policy of a policy
        set (DeviceCommunityBatch.set_policy_set, CommunityMicrogrid.evaluate_policies)."""
        return np.ascontiguousarray(self.greedy_policy(), np.uint8).reshape(-1)

    def table_stats(self) -> dict:
        """{"visited", "q_min", "q_max", "abs_max": scalars, "greedy": [n_actions] i64} of this actor's
        table (p2pmg_table_stats on the device when bound)."""
        if self._engine is None:
            return table_digest(self.q_table)[1]
        return {k: v[0] for k, v in self._engine.table_stats(first=self._slot, count=1).items()}

    def load_from_file(self, setting: str, implementation: str) -> None:
        self.set_qtable(np.load(os.path.join(MODELS_DIR, f"models_{implementation}", f"{setting}.npy")))

    def save_to_file(self, setting: str, implementation: str) -> None:
        d = os.path.join(MODELS_DIR, f"models_{implementation}")
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, f"{setting}.npy"), self.q_table)

    def save_sparse(self, path: str) -> None:
        """This actor's table as a sparse checkpoint (one table: the .npz of save_sparse_file, the format
        of DeviceCommunityBatch.save_tables).  Bound: compacted on the device (p2pmg_get_q_sparse), so
        only the stored rows travel."""
        if self._engine is None:
            save_sparse_file(path, sparse_table(self.q_table))
        else:
            self._engine.save_tables(path, first=self._slot, count=1)

    def load_sparse(self, path: str) -> None:
        """Replace the table by a one-table sparse checkpoint's (every row it does not list becomes zero)."""
        sparse = load_sparse_file(path, self._shape)
        if sparse["offsets"].size != 2:
            raise ValueError(f"{path} holds {sparse['offsets'].size - 1} tables, an actor has one")
        if self._engine is None:
            self._host_table = dense_table(sparse)[0].astype(np.float64)
        else:
            self._engine.set_q_sparse(sparse, first=self._slot, zero=True)

    # ------------------------------------------------------------ per-call API (rl.py:89-132)
    def _get_state_indices(self, state) -> Tuple[int, int, int, int]:
        eng, _ = self._device()
        idx = eng.state_indices(_as_obs(state)[:1])[0]
        return int(idx[0]), int(idx[1]), int(idx[2]), int(idx[3])

    def __call__(self, state, *args, **kwargs):
        return self.select_action(state)

    def select_action(self, state) -> Tuple[int, float]:
        if np.random.rand() < self._epsilon:
            return self.random_action()
        return self.greedy_action(state)

    def random_action(self) -> Tuple[int, float]:
        return np.random.choice(self._num_actions), 0.

    def greedy_action(self, state) -> Tuple[int, float]:
        eng, slot = self._device()
        acts, qv = eng.q_calls([slot], _as_obs(state)[:1], [255])
        return int(acts[0]), float(qv[0])

    def train(self, state, action: int, reward, next_state) -> None:
        eng, slot = self._device()
        r = reward.numpy() if hasattr(reward, "numpy") else reward
        eng.q_calls([slot], _as_obs(state)[:1], [int(action)], rewards=np.asarray(r, np.float32).ravel()[:1],
                    ns_obs=_as_obs(next_state)[:1], train=True)

    def decay_exploration(self) -> None:
        self._epsilon = max(0.1, self._decay * self._epsilon)


# ============================================================================ DQN (rl.py:135-359)
import collections  # noqa: E402
import random  # noqa: E402
from dataclasses import dataclass  # noqa: E402

random.seed(setup.seed)  # rl.py:25 seeds Python's random for select_action / sample_batch

_KERAS_SHAPES = (("kernel", (5, 64)), ("bias", (64,)), ("kernel", (64, 64)), ("bias", (64,)),
                 ("kernel", (64, 1)), ("bias", (1,)))
_N_PARAMS = 4609
_net_counter = [0]


@dataclass
class Adam:
    """Stand-in for ``tf.optimizers.Adam`` (agent.py:310): its hyper-parameters, applied on the
    device in the Keras form (oracle/dqn.py documents the update)."""
    learning_rate: float = 1e-3
    beta_1: float = 0.9
    beta_2: float = 0.999
    epsilon: float = 1e-7


def _flat(weights) -> np.ndarray:
    return np.concatenate([np.asarray(w, np.float32).ravel() for w in weights]).astype(np.float32)


def _unflat(theta) -> list:
    out, o = [], 0
    for _, shp in _KERAS_SHAPES:
        n = int(np.prod(shp))
        out.append(np.asarray(theta[o:o + n], np.float32).reshape(shp))
        o += n
    return out


class QNetwork:
    """rl.py:135-148: concat(state[4], action[1]) -> Dense(64, relu) -> Dense(64, relu) -> Dense(1).

    Weights live in a device context slot (``bind``); until then on the host.  Keras creates
    its weights lazily with glorot_uniform from TF's seed; this build draws the same
    distribution from a private NumPy stream (the global np.random is not consumed)."""

    def __init__(self):
        _net_counter[0] += 1
        from .dqn import glorot_init
        self._host = glorot_init(1, seed=setup.seed * 1000 + _net_counter[0])[0]
        self._engine, self._which, self._slot = None, "online", 0

    def bind(self, engine, which: str, slot: int) -> None:
        th = self.flat_weights()
        self._engine, self._which, self._slot = engine, which, slot
        engine.set_weights(which, th[None], first=slot)

    def unbind(self) -> None:
        self._host = self.flat_weights()
        self._engine = None

    def flat_weights(self) -> np.ndarray:
        if self._engine is None:
            return self._host.copy()
        return self._engine.get_weights(self._which, first=self._slot, count=1)[0]

    def set_flat_weights(self, theta) -> None:
        theta = np.asarray(theta, np.float32).reshape(_N_PARAMS)
        if self._engine is None:
            self._host = theta.copy()
        else:
            self._engine.set_weights(self._which, theta[None], first=self._slot)

    @property
    def trainable_weights(self) -> list:
        return _unflat(self.flat_weights())

    def get_weights(self) -> list:
        return self.trainable_weights

    def set_weights(self, weights) -> None:
        self.set_flat_weights(_flat(weights))

    def _device(self):
        if self._engine is None or self._which != "online":
            from .dqn import DeviceDQNBatch
            eng = DeviceDQNBatch(1, 1, 0, 1, device=setup.device, init_seed=None)
            eng.set_weights("online", self.flat_weights()[None])
            return eng, 0, True
        return self._engine, self._slot, False

    def __call__(self, state, action) -> np.ndarray:
        s = np.asarray(state.numpy() if hasattr(state, "numpy") else state, np.float32).reshape(-1, 4)
        a = np.asarray(action.numpy() if hasattr(action, "numpy") else action, np.float32).reshape(-1, 1)
        eng, slot, tmp = self._device()
        try:
            return eng.forward(np.concatenate([s, a], axis=1), slot)[:, None]
        finally:
            if tmp:
                eng.close()

    def save_weights(self, path: str) -> None:
        """Keras ``save_weights`` replacement: an .npz of the six arrays in Keras order."""
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        np.savez(path if path.endswith(".npz") else path + ".npz",
                 **{f"w{k}": w for k, w in enumerate(self.trainable_weights)})

    def load_weights(self, path: str) -> None:
        with np.load(path if path.endswith(".npz") else path + ".npz", allow_pickle=False) as f:
            self.set_weights([f[f"w{k}"] for k in range(6)])


class ActorModel(ActorInterface):
    """rl.py:151-197: epsilon-greedy over the action values (0, .5, 1) with a Q-network."""

    def __init__(self, epsilon: float = 0.1):
        self.actions = np.array([0., 0.5, 1.], dtype=np.float32)
        self._epsilon = epsilon
        self._decay = 0.9
        self._q_network = QNetwork()

    @property
    def q_network(self) -> QNetwork:
        return self._q_network

    def load_from_file(self, setting: str, implementation: str) -> None:
        self._q_network.load_weights(os.path.join(MODELS_DIR, f"models_{implementation}", setting))

    def save_to_file(self, setting: str, implementation: str) -> None:
        self._q_network.save_weights(os.path.join(MODELS_DIR, f"models_{implementation}", setting))

    def __call__(self, state, *args, **kwargs):
        return self.select_action(state)

    def select_action(self, state):
        if random.random() < self._epsilon:
            return self.random_action()
        return self.greedy_action(state)

    def random_action(self):
        return np.expand_dims(self.actions[np.random.choice([0, 1, 2])], axis=0), np.array([0.], np.float32)

    def greedy_action(self, state):
        s = np.asarray(state.numpy() if hasattr(state, "numpy") else state, np.float32).reshape(1, 4)
        q = self._q_network(np.repeat(s, 3, axis=0), self.actions[:, None])   # (3, 1)
        return np.expand_dims(self.actions[int(np.argmax(q[:, 0]))], axis=0), q

    def _map_engine(self, grid):
        """(engine, slot, temporary) for a map of this actor's network: its own engine on that engine's
        grid, else a one-network engine with ``grid`` (or the default)."""
        net = self._q_network
        if grid is None and net._engine is not None and net._which == "online":
            return net._engine, net._slot, False
        from .dqn import DeviceDQNBatch
        eng = DeviceDQNBatch(1, 1, 0, 1, device=setup.device, init_seed=None)  # a bound engine keeps its grid
        eng.set_weights("online", net.flat_weights()[None])
        if grid is not None:
            eng.set_policy_grid(*grid)
        return eng, 0, True

    def policy_map(self, grid=None, q: bool = False):
        """u8 (n0, n1, n2, n3): greedy_action (first maximum over the action values 0, .5, 1) at every state
        of ``grid`` = (time, temp, balance, p2p) axes; None: the bound engine's grid, else the default
        (the 20^4 table shape at its bins' centres, where byte g is row g of QActor.greedy_policy()).
        q=True: (policy, Q values f32 (n0, n1, n2, n3, 3)).  One device pass (p2pmg_dqn_policy_map)."""
        eng, slot, tmp = self._map_engine(grid)
        try:
            out = eng.policy_map(first=slot, count=1, q=q)
            return (out[0][0], out[1][0]) if q else out[0]
        finally:
            if tmp:
                eng.close()

    def map_stats(self, grid=None) -> dict:
        """{"states", "q_min", "q_max", "abs_max", "min_gap": scalars, "greedy": [3] i64} of this actor's
        network over the grid (p2pmg_dqn_map_stats)."""
        eng, slot, tmp = self._map_engine(grid)
        try:
            return {k: v[0] for k, v in eng.map_stats(first=slot, count=1).items()}
        finally:
            if tmp:
                eng.close()

    def decay_exploration(self) -> None:
        self._epsilon *= self._decay  # no floor for the DQN actor (rl.py:196-197)


class ReplayBuffer:
    """rl.py:200-248.  Host deque for standalone use; inside a community the memory is the
    device ring of the agent (``bind``) and sampling reads it back."""

    def __init__(self, buffer_size: int, batch_size: int):
        self.buffer_size = buffer_size
        self.batch_size = batch_size
        self.count = 0
        self.buffer = collections.deque(maxlen=buffer_size)
        self._engine, self._slot = None, 0

    def bind(self, engine, slot: int) -> None:
        self._engine, self._slot = engine, slot

    def _device_rows(self):
        ring, added = self._engine.get_buffer(self._slot, 1)
        n = int(added[0])
        cnt = min(n, self.buffer_size)
        order = (n - cnt + np.arange(cnt)) % self.buffer_size
        return ring[0][order]

    def add(self, s, a, r, ns) -> None:
        if self._engine is not None:
            raise RuntimeError("this agent's memory is device-resident (filled by the community kernels)")
        self.count = min(self.count + 1, self.buffer_size)
        self.buffer.append((s, a, r, ns))

    def add_batch(self, s, a, r, ns) -> None:
        for i in range(np.shape(s)[0]):
            self.add(s[i, :], a[i], r[i], ns[i, :])

    def size(self) -> int:
        if self._engine is not None:
            return len(self._device_rows())
        return min(self.count, self.buffer_size)

    def sample_batch(self):
        if self._engine is not None:
            rows = self._device_rows()
            idx = random.sample(range(len(rows)), min(len(rows), self.batch_size))
            b = rows[idx]
            return b[:, 0:4], b[:, 4:5], b[:, 5:6], b[:, 6:10]
        batch = random.sample(self.buffer, min(self.count, self.batch_size))
        return tuple(np.stack([np.asarray(x[k], np.float32) for x in batch]) for k in range(4))

    def clear(self):
        self.buffer.clear()
        self.count = 0


class Trainer:
    """rl.py:251-359: TD targets from a target network, MSE loss, first-kernel gradient clip,
    Adam, soft target update - one device launch per ``train`` (p2pmg_dqn_train_batch)."""

    def __init__(self, actor: ActorModel, buffer_size: int, batch_size: int, gamma: float, tau: float,
                 optimizer: Adam):
        self._batch_size = batch_size
        self._gamma = gamma
        self._tau = tau
        self.actor = actor
        self.target_network = ActorModel().q_network
        self.optimizer = optimizer
        self.buffer = ReplayBuffer(buffer_size, batch_size)
        self._engine, self._slot = None, 0

    def bind(self, engine, slot: int) -> None:
        """Attach actor (online), target network and memory to agent ``slot`` of a DeviceDQNBatch."""
        self.actor.q_network.bind(engine, "online", slot)
        self.target_network.bind(engine, "target", slot)
        self.buffer.bind(engine, slot)
        self._engine, self._slot = engine, slot
        # this trainer's own gamma, tau and Adam learning rate (rl.py:253-266) into its network's row of the
        # engine's per-network arrays (a slot is a network where every agent has its own; a shared network
        # keeps the engine's values)
        if engine.n_nets == engine.A:
            cur = engine.get_learning()
            g, t, lr = (cur[k].reshape(-1) for k in ("gamma", "tau", "lr"))
            mine = (float(self._gamma), float(self._tau), float(self.optimizer.learning_rate))
            if (g[slot], t[slot], lr[slot]) != mine:
                g[slot], t[slot], lr[slot] = mine
                engine.set_learning(gamma=g, tau=t, lr=lr)

    def _device(self):
        if self._engine is None:
            from .dqn import DeviceDQNBatch
            eng = DeviceDQNBatch(1, 1, 0, 1, device=setup.device, gamma=self._gamma, tau=self._tau,
                                 lr=self.optimizer.learning_rate, capacity=self.buffer.buffer_size, init_seed=None)
            self.actor.q_network.bind(eng, "online", 0)
            self.target_network.bind(eng, "target", 0)
            self._engine, self._slot = eng, 0
        return self._engine, self._slot

    def initialize_target(self) -> None:
        self.buffer.sample_batch()  # the reference draws a batch to build the Keras models (rl.py:275)
        self._soft_update(self.actor.q_network, self.target_network, tau=1.0)

    def load_from_file(self, setting: str, implementation: str) -> None:
        self.target_network.load_weights(os.path.join(MODELS_DIR, f"models_{implementation}", f"{setting}_target"))

    def save_to_file(self, setting: str, implementation: str) -> None:
        self.target_network.save_weights(os.path.join(MODELS_DIR, f"models_{implementation}", f"{setting}_target"))

    def train(self) -> float:
        s, a, r, ns = self.buffer.sample_batch()
        return self._train(s, a, r, ns)

    def _train(self, states, actions, rewards, next_states) -> float:
        """One Trainer._train + update_targets on the device (the soft update is fused)."""
        eng, slot = self._device()
        return eng.train_batch(states, actions, rewards, next_states, net=slot)

    def _soft_update(self, source: QNetwork, target: QNetwork, tau: float = 1.0) -> None:
        ts, tt = source.flat_weights(), target.flat_weights()
        target.set_flat_weights(ts if tau == 1.0 else (np.float32(1 - tau) * tt + np.float32(tau) * ts))

    def update_targets(self) -> None:
        """Applied inside every device train step (rl.py:356-359 follows each _train)."""
