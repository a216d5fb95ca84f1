"""Cases, weights and inputs shared by the DQN evaluation tests (test_cpu_dqn_eval.py checks them on the
oracle without a GPU, test_gpu_dqn_eval.py runs them on the device).

A case is (S, N, R, T) with the seed and scale of its networks.  The seeds and scales are chosen so that the
greedy policy is not constant: every action 0, 1 and 2 occurs in the action record of
``OracleDQNBatch(order="device").run_episode("greedy")`` (``oracle_actions``), which keeps a constant policy
from hiding a wrong network index or a wrong W2 column.  One case cannot show three actions: N = 1 at T = 1
with S = 2 has two decisions in all (a lone agent's proposal matrix is its zeroed diagonal, so its
observation, and with it its action, is the same in every round); it is held to the two it can show
(``actions_needed``).  Pure NumPy."""
from collections import namedtuple

import numpy as np

from oracle import dqn as odqn
from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.dqn import glorot_init

F32 = np.float32
RECORDS = ("reward", "cost", "grid", "p2p", "t_in", "action")

# n_env: "S" = one environment row per scenario, 1 = one shared row; shared: one network for every agent
# (the other side is then the MFMA act kernel); mixed: per-agent heat-pump levels and {setpoint, lower,
# upper, cop} away from the defaults
Case = namedtuple("Case", "S N R T seed scale n_env shared mixed")
CASES = {
    "s3n2r1t12": Case(3, 2, 1, 12, 0, 8.0, "S", False, False),
    "s2n3r0t5_odd_T": Case(2, 3, 0, 5, 0, 8.0, 1, False, True),
    "s2n1r2t1": Case(2, 1, 2, 1, 0, 8.0, "S", False, False),
    "s2n8r1t4": Case(2, 8, 1, 4, 0, 8.0, "S", False, False),
    "s2n16r1t3_1024_threads": Case(2, 16, 1, 3, 0, 8.0, "S", False, False),
    "s2n9r2t3_wide16": Case(2, 9, 2, 3, 0, 8.0, "S", False, False),
    "s2n17r1t3_wide32": Case(2, 17, 1, 3, 0, 8.0, "S", False, True),
    "s1n64r0t2_wide64": Case(1, 64, 0, 2, 0, 8.0, "S", False, False),
    "s3n2r1t12_shared_net": Case(3, 2, 1, 12, 5, 8.0, "S", True, False),
}
# the policy-set tests: M networks for (S, N)
ROLE = Case(4, 3, 1, 6, 0, 8.0, "S", False, False)      # M = N = 3, the role map
ARBITRARY = Case(3, 2, 1, 6, 2, 8.0, "S", False, False)  # A = 6, M = 2
ARBITRARY_MAP = np.array([1, 0, 0, 1, 1, 0], np.int32)


def weights(n_nets, seed, scale):
    """Glorot kernels with the (zero) biases overwritten by small random values, all times ``scale``."""
    th = glorot_init(n_nets, seed)
    rs = np.random.RandomState(1000 + seed)
    for lo, hi in ((320, 384), (4480, 4544), (4608, 4609)):
        th[:, lo:hi] = rs.uniform(-0.1, 0.1, (n_nets, hi - lo)).astype(F32)
    return (th * F32(scale)).astype(F32)


def case_weights(c):
    """The case's own networks: one per agent, or the one shared network."""
    return weights(1 if c.shared else c.S * c.N, c.seed, c.scale)


def inputs(c):
    return scenario_batch(c.S, c.N, c.T, shared_weather=c.n_env == 1)


def thermal(c):
    """(levels [S, N, 3], params [S, N, 4] = {setpoint, lower, upper, cop}) f32: mixed values per agent, or
    None for the defaults."""
    if not c.mixed:
        return None
    a = np.arange(c.S * c.N)
    power = np.array([2000.0, 3000.0, 4500.0, 1500.0], F32)[a % 4]
    levels = (np.array([0.0, 0.5, 1.0], F32)[None, :] * power[:, None]).astype(F32)
    sp = np.array([20.0, 21.0, 22.5], F32)[a % 3]
    lower = (sp - np.array([1.0, 0.5], F32)[a % 2]).astype(F32)
    upper = (sp + np.array([1.0, 1.5, 0.75], F32)[(a // 2) % 3]).astype(F32)
    cop = np.array([2.5, 3.0, 3.5, 4.0, 2.0], F32)[a % 5]
    return levels.reshape(c.S, c.N, 3), np.stack([sp, lower, upper, cop], -1).reshape(c.S, c.N, 4)


def load(eng, c, inp=None):
    """Upload the case's inputs, start temperatures and thermal values into a DeviceDQNBatch."""
    inp = inputs(c) if inp is None else inp
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    th = thermal(c)
    if th is not None:
        eng.set_hp_levels(th[0])
        eng.set_thermal(th[1][..., 0], cop=th[1][..., 3], lower=th[1][..., 1], upper=th[1][..., 2])
    return inp


def oracle_batch(c, theta):
    """The oracle of the case (default thermal values) with networks ``theta``: [A, 4609], or [1, 4609]
    for a shared network."""
    inp = inputs(c)
    ob = odqn.OracleDQNBatch(S=c.S, N=c.N, R=c.R, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in,
                             env_time=inp.time[None], env_tout=inp.t_out, theta0=theta, shared=c.shared)
    ob.t_in, ob.t_m = inp.t_in0.copy(), inp.t_m0.copy()
    return ob


def oracle_actions(c, theta):
    return oracle_batch(c, theta).run_episode("greedy")["action"]


def actions_needed(c):
    """How many of the three actions a case's record can and must show."""
    return min(3, c.S * c.T) if c.N == 1 else 3


def tiled(theta, S):
    """[M, 4609] role networks -> [S * M, 4609]: network i of every scenario."""
    return np.tile(theta, (S, 1))


def default_map_cases():
    """(count, S, N, expected map or None = raises) for the default-map rule."""
    return [(3, 4, 3, np.arange(12) % 3), (12, 4, 3, np.arange(12)), (1, 4, 3, np.zeros(12, int)),
            (2, 1, 2, np.arange(2)), (1, 1, 1, np.zeros(1, int)), (2, 4, 3, None), (4, 4, 3, None), (0, 4, 3, None)]
