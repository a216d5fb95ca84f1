"""Helpers of the policy-set tests (tests/test_cpu_policy_set.py, tests/test_gpu_policy_set.py,
tests/test_gpu_policy_set_api.py).

The reference of p2pmg_run_policy is the unchanged OracleBatch in mode="greedy" whose agent a holds the ONE-HOT
table of its policy: entry [row, b] = 1 where b is the row's byte, and an all-zero row for byte 255.  The
oracle's first-maximum argmax of such a row is the byte (0 for 255), which is the action the device takes.
"""
import functools

import numpy as np

from oracle.restatement import OracleBatch, OracleParams
from p2pmicrogrid_amd.dataset import scenario_batch

F32 = np.float32
UNVISITED = 255
REC = ["reward", "cost", "grid", "p2p", "t_in", "action", "index"]
BYTES = np.array([0, 1, 2, UNVISITED], np.uint8)


def action_of(policy):
    """The action each byte stands for: the byte, and 0 for 255."""
    p = np.asarray(policy, np.uint8)
    return np.where(p == UNVISITED, 0, p).astype(np.int64)


def random_policies(M, n_states, seed):
    """u8 [M, n_states], uniform over {0, 1, 2, 255}."""
    return BYTES[np.random.RandomState(seed).randint(0, 4, (M, n_states))]


def one_hot_tables(policies, n_actions=3, dtype=np.float32, alt=False):
    """[M, n_states, n_actions]: 1 at [row, byte], nothing for 255.  alt: another table set with the same packed
    policy (the greedy entry 2.5, a smaller positive entry after it where there is room, negative ones before)."""
    p = np.asarray(policies, np.uint8)
    M, n = p.shape
    q = np.zeros((M, n, n_actions), dtype)
    m, r = np.nonzero(p != UNVISITED)
    b = p[m, r].astype(np.int64)
    if alt:
        for k in range(n_actions):
            q[m, r, k] = np.where(k < b, -1.0 - k, np.where(k == b, 2.5, 0.25))
    else:
        q[m, r, b] = 1
    return q


def draw_thermal(S, N, seed=99):
    """Per-agent setpoint, COP [S, N] f64 (exact in f32) and heat-pump levels [S, N, 3] f32."""
    rs = np.random.RandomState(seed)
    sp = rs.choice((19.5, 21.0, 22.0, 23.25), (S, N))
    cop = rs.choice((2.5, 3.0, 4.0), (S, N))
    mp = rs.choice((2e3, 3e3, 5e3), (S, N))
    lv = np.stack([(l * mp).astype(F32) for l in (0.0, 0.5, 1.0)], axis=-1)
    return sp, cop, lv


def mixed_capacities(S, N, seed=5):
    """Battery capacities [S, N] J, about half of them 0 (no battery)."""
    rs = np.random.RandomState(seed)
    cap = rs.choice((0.0, 3.6e6, 7.2e6), (S, N))
    cap.flat[0], cap.flat[-1] = 0.0, 7.2e6
    return cap


def inputs(S, N, T, seed=11):
    return scenario_batch(S, N, T, seed=seed)


def oracle_for(inp, N, R, tables, dims=None, thermal=None, battery=None):
    """An OracleBatch on inp whose per-agent tables are `tables` [A, n_states, 3]."""
    S = inp.load_w.shape[0]
    kw, pk = {}, {}
    if dims is not None:
        pk.update(n_time=dims[0], n_temp=dims[1], n_bal=dims[2], n_p2p=dims[3])
    if thermal is not None:
        pk.update(setpoint=thermal[0], hp_cop=thermal[1])
        kw["hp_levels"] = thermal[2]
    if battery is not None:
        kw["battery_capacity"] = battery
    ob = OracleBatch(S=S, N=N, R=R, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in, env_time=inp.time[None],
                     env_tout=inp.t_out, q_dtype="f32", params=OracleParams(**pk), **kw)
    assert tables.shape == (S * N, ob.n_states, 3)
    ob.q = tables
    ob.t_in, ob.t_m = inp.t_in0.copy(), inp.t_m0.copy()
    return ob


def oracle_policy_run(inp, N, R, policies, policy_of, **kw):
    """The oracle's greedy run with agent a on the one-hot table of policies[policy_of[a]]."""
    tables = one_hot_tables(np.asarray(policies)[np.asarray(policy_of).reshape(-1)])
    ob = oracle_for(inp, N, R, tables, **kw)
    out = ob.run_episode("greedy")
    if kw.get("battery") is not None:
        out["soc_final"] = ob.soc.copy()
    return out


@functools.lru_cache(maxsize=None)
def reference(S, N, R, T, dims=None, thermal=False, battery=False, seed=11):
    """One case of test 1, computed once and shared (nothing downstream modifies it): inputs, M == A random
    policies, the per-agent extras and the oracle's run."""
    inp = inputs(S, N, T, seed)
    n_states = int(np.prod(dims)) if dims else 160000
    pol = random_policies(S * N, n_states, seed=1000 + 31 * S + N)
    th = draw_thermal(S, N) if thermal else None
    cap = mixed_capacities(S, N) if battery else None
    out = oracle_policy_run(inp, N, R, pol, np.arange(S * N), dims=dims, thermal=th, battery=cap)
    return inp, pol, th, cap, out


def device_for(inp, N, R, dims=None, thermal=None, battery=None, **kw):
    """A shared_q=True engine (one table, which run_policy never reads) on inp."""
    from p2pmicrogrid_amd.engine import DeviceCommunityBatch
    S, T = inp.load_w.shape[0], inp.load_w.shape[-1]
    if dims is not None:
        kw.update(n_time_states=dims[0], n_temp_states=dims[1], n_balance_states=dims[2], n_p2p_states=dims[3])
    kw.setdefault("shared_q", True)
    kw.setdefault("q_dtype", "f32")
    eng = DeviceCommunityBatch(S, N, R, T, **kw)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    if thermal is not None:
        eng.set_hp_levels(thermal[2])
        eng.set_thermal(thermal[0], thermal[1])
    if battery is not None:
        eng.set_battery(battery)
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    return eng


# ----------------------------------------------------------------- the object API (evaluate_policies)
DAY_KEYS = ("power", "cost", "decisions", "t_in", "t_in_final", "t_m_final")


def dqn_community(n_agents, seed=7, scale=8.0):
    """get_community(DQNAgent, n) with seeded, scaled weights written into the agents (tests/dqn_eval_cases.py):
    a policy that takes every action on the test days."""
    import dqn_eval_cases as dc
    from p2pmicrogrid_amd import community
    from p2pmicrogrid_amd.agent import DQNAgent
    np.random.seed(42)
    com = community.get_community(DQNAgent, n_agents)
    for a, th in zip(com.agents, dc.weights(n_agents, seed, scale)):
        a.actor.q_network.set_flat_weights(th)
    return com


def day_inputs(com, D, T, seed=31):
    """Scenario inputs of D days of T steps with the community's own max_in."""
    import summary_cases
    N = len(com.agents)
    inp = summary_cases.batch_inputs(D, N, T, seed=seed)
    inp.max_in = np.broadcast_to(np.array([F32(a.max_in) for a in com.agents], F32), (D, N)).copy()
    return inp


def days_of(inp):
    """evaluate_days' / evaluate_policies' `days` argument from scenario inputs."""
    return [{"time": inp.time, "t_out": inp.t_out[d], "load": inp.load_w[d], "pv": inp.pv_w[d], "t_in": inp.t_in0[d],
             "t_m": inp.t_m0[d]} for d in range(inp.load_w.shape[0])]


def assert_same_day(got, want, tag):
    for k in DAY_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (tag, k)
        assert np.array_equal(got[k], want[k]), (tag, k)


def assert_records_equal(rec, out, tag=""):
    """get_records(REC) of a device run against an oracle output, bit for bit."""
    from p2pmicrogrid_amd.engine import unpack_index
    for k in ("reward", "cost", "grid", "p2p", "t_in"):
        assert np.array_equal(rec[k], out[k]), (tag, k)
    assert np.array_equal(rec["action"], out["action"].astype(np.uint8)), (tag, "action")
    assert np.array_equal(unpack_index(rec["index"]), out["idx"]), (tag, "index")


def assert_state_equal(eng, out, tag=""):
    t_in, t_m = eng.get_temperatures()
    assert np.array_equal(t_in, out["t_in_final"]) and np.array_equal(t_m, out["t_m_final"]), (tag, "temperatures")
    assert np.array_equal(eng.episode_reward(), out["episode_reward"]), (tag, "episode reward")
    if "soc_final" in out:
        assert np.array_equal(eng.get_soc(), out["soc_final"]), (tag, "soc")
