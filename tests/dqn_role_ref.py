"""Reference for one DQN network per ROLE (p2pmg_dqn_setup_roles, DeviceDQNBatch(shared="role")): the oracle's own
pieces (oracle.dqn.block_layout, train_block, fold_segments, sum_segments, adam_step, soft_update and
OracleDQNBatch's episode loop) called per role.  TEST INFRASTRUCTURE ONLY.

RoleDQNBatch holds N networks ([N, 4609] arrays); agent (s, i) of every scenario acts on network i.  Per training
env step and role i, in the device's order: the role's agents k N + i, k = 0..S-1, in blocks of agents_per_block
consecutive scenarios (block_layout(S, 1, apb)), one train_block partial per block, the partials folded as
dqn_reduce_adam_kernel folds them (fold_segments, one segment), times F32(1) / F32(S), then adam_step and the soft
update on row i with the role's own DQNParams.  It hooks the oracle's episode loop where MixedDQNBatch
(tests/dqn_learning_ref.py) does: _nets, _train_device and, for the duration of run_episode, the module-level
soft_update.  It restates the device order only.  At N = 1 it is OracleDQNBatch(shared=True), at S = 1 the
per-agent OracleDQNBatch, bit for bit (tests/test_cpu_dqn_roles.py)."""
from dataclasses import dataclass, replace

import numpy as np

from oracle import dqn as odqn

F32 = np.float32


def preload_rings(n_agents: int, capacity: int, held: int, seed: int = 3):
    """(ring [A, capacity, 10] f32, added [A] int32): `held` transitions per agent already in memory, values in
    (-1, 1) from a NumPy seed.  A training episode is admitted only with 31 transitions per agent in memory
    (p2pmg_run_episode: one more is appended before the first sample of 32), which one fill episode of a
    short test horizon does not give; DeviceDQNBatch.set_buffer / load_rings put these in first."""
    rs = np.random.RandomState(seed)
    ring = np.zeros((n_agents, capacity, 10), F32)
    ring[:, :held] = rs.uniform(-1.0, 1.0, size=(n_agents, held, 10)).astype(F32)
    return ring, np.full(n_agents, held, np.int32)


def load_rings(ob, ring, added):
    """The same memory into an OracleDQNBatch (or RoleDQNBatch)."""
    ob.buf = np.asarray(ring, F32).reshape(ob.S, ob.N, -1, 10).copy()
    ob.added = np.asarray(added, np.int64).reshape(ob.S, ob.N).copy()


@dataclass
class RoleDQNBatch(odqn.OracleDQNBatch):
    def __post_init__(self):
        if self.shared:
            raise ValueError("RoleDQNBatch: shared stays False (the N role networks are its own layout)")
        if self.grad_segments != 1 or self.world != 1:
            raise ValueError("RoleDQNBatch: one gradient segment on one rank")
        theta0 = np.asarray(self.theta0, F32).reshape(-1, odqn.N_PARAMS)
        if theta0.shape[0] != self.N:
            raise ValueError(f"RoleDQNBatch: theta0 holds one network per role ({self.N}), got {theta0.shape[0]}")
        self.theta0 = np.zeros((1, odqn.N_PARAMS), F32)  # the base class lays out S * N rows: replaced below
        super().__post_init__()
        self.theta0 = theta0
        self.theta = theta0.copy()
        self.target = theta0.copy()
        self.m = np.zeros_like(self.theta)
        self.v = np.zeros_like(self.theta)
        self.base_dqn, self.base_weight = self.dqn, self.params.penalty_weight
        self.set_learning()

    def set_learning(self, gamma=None, tau=None, lr=None, clip=None, penalty_weight=None):
        """DeviceDQNBatch.set_learning on a role batch: gamma, tau, lr, clip broadcast to [N] (one row per role),
        penalty_weight to [S, N]; None leaves a field, all None restores the constructor's."""
        if all(x is None for x in (gamma, tau, lr, clip, penalty_weight)):
            self.role_dqn = [self.base_dqn] * self.N
            self.params = replace(self.params, penalty_weight=self.base_weight)
            return
        for name, x in (("gamma", gamma), ("tau", tau), ("lr", lr), ("clip", clip)):
            if x is not None:
                v = np.broadcast_to(np.asarray(x, np.float64), (self.N,))
                self.role_dqn = [replace(d, **{name: float(v[i])}) for i, d in enumerate(self.role_dqn)]
        if penalty_weight is not None:
            w = np.ascontiguousarray(np.broadcast_to(np.asarray(penalty_weight, F32), (self.S, self.N)))
            self.params = replace(self.params, penalty_weight=w)

    def get_learning(self):
        out = {k: np.array([getattr(d, k) for d in self.role_dqn], np.float64) for k in ("gamma", "tau", "lr", "clip")}
        out["penalty_weight"] = np.ascontiguousarray(
            np.broadcast_to(np.asarray(self.params.penalty_weight, F32), (self.S, self.N)))
        return out

    def _nets(self, x):
        """Row i for agent i of every scenario: [N, ...] -> [S, N, ...]."""
        return np.broadcast_to(x[None], (self.S,) + x.shape)

    def _train_device(self, b, dp):
        S, N = self.S, self.N
        ls = np.zeros(b.shape[0], F32)
        _, apb, bps, blocks = odqn.block_layout(S, 1, self.agents_per_block)
        counts = np.array([n for _, n in blocks])
        for i, dk in enumerate(self.role_dqn):
            bi = b[i::N]  # the role's agents k N + i in scenario order
            bb = np.zeros((len(blocks), apb) + b.shape[1:], F32)
            for j, (k0, n) in enumerate(blocks):
                bb[j, :n] = bi[k0:k0 + n]
            partials, lb = odqn.train_block(self.theta[i], self.target[i], bb, dk.gamma, counts)
            ls[i::N] = np.concatenate([lb[j, :n] for j, (_, n) in enumerate(blocks)])
            grad = odqn.sum_segments(odqn.fold_segments(partials, bps)) * (F32(1) / F32(S))
            step = np.asarray(self.step)[i:i + 1] if np.ndim(self.step) else self.step
            odqn.adam_step(self.theta[i:i + 1], self.m[i:i + 1], self.v[i:i + 1], grad[None], step, dk)
        return ls

    def run_episode(self, *args, **kw):
        if self.order != "device":
            raise ValueError("RoleDQNBatch restates the device order only")
        one = odqn.soft_update

        def per_role(target, theta, tau):
            for i, dk in enumerate(self.role_dqn):
                one(target[i], theta[i], dk.tau)

        odqn.soft_update = per_role
        try:
            return super().run_episode(*args, **kw)
        finally:
            odqn.soft_update = one
