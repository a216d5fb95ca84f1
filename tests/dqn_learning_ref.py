"""Reference for per-network DQN learner constants inside one batch (p2pmg_dqn_set_learning): the oracle's
own pieces (oracle.dqn.train_block, adam_lr / adam_step, soft_update, OracleDQNBatch's episode loop) called
per network with that network's DQNParams.  TEST INFRASTRUCTURE ONLY.

OracleDQNBatch trains every per-agent network with one DQNParams.  MixedDQNBatch keeps one DQNParams per
network and one comfort weight per agent, and hooks the oracle's episode loop in two places:
  * _train_device (the per-agent branch) runs train_block + adam_step for the networks of each distinct
    DQNParams, with that gamma, clip and lr and each network's own Adam iteration count;
  * the loop's module-level soft_update call is replaced, for the duration of run_episode, by one that applies
    oracle.dqn.soft_update row by row with the network's own tau.
The comfort weight goes in as OracleParams.penalty_weight [S, N], which oracle.restatement.reward broadcasts.
With equal values everywhere it is OracleDQNBatch bit for bit (tests/test_cpu_dqn_learning.py).
per_scenario_eps() lets either batch run one Philox episode with a rate per scenario."""
from contextlib import contextmanager
from dataclasses import astuple, dataclass, replace

import numpy as np

from oracle import dqn as odqn
from oracle import philox

F32 = np.float32


@contextmanager
def per_scenario_eps():
    """Inside: OracleDQNBatch.run_episode(rng="philox", eps=[S, 1] or [S, N]) takes rates that differ between
    agents (p2pmg_dqn_run_episode_eps).  The oracle draws a launch's decisions with one epsilon
    (philox.launch_eps refuses more); here the draws of each distinct rate's agents come from the oracle's own
    philox.decision_draws at that rate, so every agent explores as in a launch at its rate."""
    one_eps, draws = philox.launch_eps, philox.decision_draws

    def decision_draws(seed, episode, agents, t, r, rounds, eps=None):
        agents = np.asarray(agents)
        e = np.broadcast_to(np.asarray(eps, np.float64), agents.shape)
        u, act = np.zeros(agents.shape, np.float64), np.zeros(agents.shape, np.int64)
        for v in np.unique(e):
            m = e == v
            u[m], act[m] = draws(seed, episode, agents[m], t, r, rounds, eps=float(v))
        return u, act

    philox.launch_eps = lambda eps_arr: np.asarray(eps_arr, np.float64).ravel()
    philox.decision_draws = decision_draws
    try:
        yield
    finally:
        philox.launch_eps, philox.decision_draws = one_eps, draws


@dataclass
class MixedDQNBatch(odqn.OracleDQNBatch):
    def __post_init__(self):
        if self.shared:
            raise ValueError("MixedDQNBatch: per-agent networks (a shared network has one row: OracleDQNBatch)")
        super().__post_init__()
        self.base_dqn, self.base_weight = self.dqn, self.params.penalty_weight
        self.set_learning()

    def set_learning(self, gamma=None, tau=None, lr=None, clip=None, penalty_weight=None):
        """DeviceDQNBatch.set_learning: values broadcast to [S, N]; None leaves a field, all None restores."""
        A, shape = self.S * self.N, (self.S, self.N)
        if all(x is None for x in (gamma, tau, lr, clip, penalty_weight)):
            self.net_dqn = [self.base_dqn] * A
            self.params = replace(self.params, penalty_weight=self.base_weight)
            return
        for name, x in (("gamma", gamma), ("tau", tau), ("lr", lr), ("clip", clip)):
            if x is not None:
                v = np.broadcast_to(np.asarray(x, np.float64), shape).reshape(A)
                self.net_dqn = [replace(d, **{name: float(v[k])}) for k, d in enumerate(self.net_dqn)]
        if penalty_weight is not None:
            w = np.ascontiguousarray(np.broadcast_to(np.asarray(penalty_weight, F32), shape))
            self.params = replace(self.params, penalty_weight=w)

    def get_learning(self):
        shape = (self.S, self.N)
        out = {k: np.array([getattr(d, k) for d in self.net_dqn], np.float64).reshape(shape)
               for k in ("gamma", "tau", "lr", "clip")}
        out["penalty_weight"] = np.ascontiguousarray(np.broadcast_to(np.asarray(self.params.penalty_weight, F32), shape))
        return out

    def _train_device(self, b, dp):
        ls = np.zeros(b.shape[0], F32)
        groups = {}  # the networks of each distinct DQNParams go through the oracle's calls together (row-wise ops)
        for k, dk in enumerate(self.net_dqn):
            groups.setdefault(astuple(dk), (dk, []))[1].append(k)
        for dk, idx in groups.values():
            th, m, v = self.theta[idx], self.m[idx], self.v[idx]
            gr, lk = odqn.train_block(th, self.target[idx], b[idx][:, None], dk.gamma)
            step = np.asarray(self.step)[idx] if np.ndim(self.step) else self.step
            odqn.adam_step(th, m, v, gr, step, dk)
            self.theta[idx], self.m[idx], self.v[idx] = th, m, v
            ls[idx] = lk[:, 0]
        return ls

    def run_episode(self, *args, **kw):
        if self.order != "device":
            raise ValueError("MixedDQNBatch restates the device order only")
        one = odqn.soft_update

        def per_network(target, theta, tau):
            for k, dk in enumerate(self.net_dqn):
                one(target[k], theta[k], dk.tau)

        odqn.soft_update = per_network
        try:
            return super().run_episode(*args, **kw)
        finally:
            odqn.soft_update = one
