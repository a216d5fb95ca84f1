"""The interleaved chain's undo log for step T - 1's next-state row: the first time
the follower episode stores into a row (key of step 0, temperature bin, p2p = 0) it logs what it
read there, and the leader's step T - 1 takes its TD target from the log where the follower has
written and from its own loaded row elsewhere.  Every case runs S = 20, N = 2 and at most six
episodes per chain (the 70-episode call aside), interleaved, and compares it bit for bit with one
launch per episode AND with the oracle: tables, the last episode's records, every episode's reward
and the final temperatures.
"""
import dataclasses

import numpy as np
import pytest

from oracle import philox
from oracle.restatement import OracleBatch, OracleParams
from p2pmicrogrid_amd.engine import unpack_index
from test_gpu_chain_interleave import F32, WIDE, _engine, _inputs, _keys, _lag, _schedule

pytestmark = pytest.mark.gpu

S, N = 20, 2
SEED = 42  # the engine's default seed
SETPOINTS = (19.5, 21.0, 22.0, 23.25)  # exact in f32: the oracle's f64 T0 equals the device's


def _oracle(inp, R, q, setpoint=None, **cfg):
    par = OracleParams(n_time=cfg.get("n_time_states", 20), n_temp=cfg.get("n_temp_states", 20),
                       n_bal=cfg.get("n_balance_states", 20), n_p2p=cfg.get("n_p2p_states", 20))
    if setpoint is not None:
        par = dataclasses.replace(par, setpoint=setpoint)
    ob = OracleBatch(S=S, N=N, R=R, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in,
                     env_time=np.asarray(inp.time, F32).reshape(1, -1), env_tout=inp.t_out, q_dtype=q, params=par)
    ob.t_in, ob.t_m = inp.t_in0.copy(), inp.t_m0.copy()
    return ob


def _oracle_run(ob, e0, eps, sigma):
    """Episodes e0 .. of the chain on the oracle, each followed by the T0 reset (community.py:181);
    -> every episode's reward and the last episode's records."""
    rew, out = [], None
    sp = np.broadcast_to(np.asarray(ob.params.setpoint, np.float64), (S, N)).ravel()
    for k, x in enumerate(eps):
        out = ob.run_episode("train", rng="philox", seed=SEED, episode=e0 + k, eps=x)
        rew.append(out["episode_reward"])
        t_in, t_m = philox.t0_draws(SEED, e0 + k + 1, np.arange(S * N), setpoint=sp, sigma=sigma)
        ob.t_in, ob.t_m = t_in.reshape(S, N), t_m.reshape(S, N)
    return np.stack(rew), out


def _singles(eng, e0, eps, sigma):
    rew = []
    for k, x in enumerate(eps):
        eng.run_episode("train", "philox", episode=e0 + k, epsilon=x, reset_sigma=sigma, record=WIDE,
                        next_epsilon=eps[k + 1] if k + 1 < len(eps) else None)
        rew.append(eng.episode_reward())
    return np.stack(rew)


def _chain(eng, e0, eps, sigma):
    eng.run_episodes(e0, eps, reset_sigma=sigma, record=WIDE)
    name = eng.last_kernel()
    assert name.startswith("episode_fast_kernel<") and name.endswith(",interleaved>"), name
    return eng.episode_rewards()


def _same(chain, single, ob, out, q):
    """The interleaved chain's state against the single launches' and the oracle's."""
    qt = np.float64 if q == "f64" else np.float32
    tq = chain.get_q(dtype=qt)
    assert np.array_equal(tq, single.get_q(dtype=qt))
    assert np.array_equal(tq.reshape(S * N, -1, 3), ob.q)
    for x, y, z in zip(chain.get_temperatures(), single.get_temperatures(), (ob.t_in, ob.t_m)):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    rc, rs = chain.get_records(WIDE), single.get_records(WIDE)
    for k in WIDE:
        assert np.array_equal(rc[k], rs[k]), k
    for k in ("reward", "cost", "grid", "p2p", "t_in"):
        assert np.array_equal(rc[k], out[k]), k
    assert np.array_equal(rc["action"], out["action"].astype(np.uint8))
    assert np.array_equal(unpack_index(rc["index"]), out["idx"])


def _check(inp, R, q, eps, e0=2, sigma=0.3, **cfg):
    """-> (D, safe) of the inputs, after the three-way comparison."""
    ob = _oracle(inp, R, q, **cfg)
    want, out = _oracle_run(ob, e0, eps, sigma)
    single, chain = _engine(inp, N, R, q, **cfg), _engine(inp, N, R, q, **cfg)
    rs = _singles(single, e0, eps, sigma)
    rc = _chain(chain, e0, eps, sigma)
    assert np.array_equal(rc, rs) and np.array_equal(rc, want)
    _same(chain, single, ob, out, q)
    lag = chain.chain_lag()
    assert lag[0] == _lag(*_keys(chain, inp))
    single.close()
    chain.close()
    return lag


# ------------------------------------------------------------------ 1. repeated writes to one entry
def _shared_key_day(d, T=48, n_time=6):
    """Constant balances (the key is the time bin alone) and a time column whose steps 0 .. d fall
    into time bin 0 and the rest, in order, into bins 1 .. n_time - 1: the only keys d apart are
    steps 0 and d of bin 0 (lo-lo), so D = d, and every step 0 .. d stores into rows of step 0's key."""
    rest = np.array_split(np.arange(d + 1, T), n_time - 1)
    time = np.empty(T)
    for b, steps in enumerate([np.arange(d + 1)] + rest):
        time[steps] = (b + (np.arange(len(steps)) + 0.5) / len(steps)) / n_time
    inp = _inputs(S, N, T, time=time)
    load = np.broadcast_to((0.3 * inp.max_in)[..., None], inp.load_w.shape).astype(F32)
    return dataclasses.replace(inp, load_w=np.ascontiguousarray(load), pv_w=np.zeros_like(load))


@pytest.mark.parametrize("R", [0, 1])
def test_repeated_writes_to_one_entry_at_the_threshold(R):
    """A 6 x 2 x 2 x 2 table, T = 48 (L = 24), mostly greedy, steps 0 .. 20 on step 0's key: D = 20,
    D + 4 = L, the last accepted distance.  The follower stores 21 times into the two p2p = 0 rows of
    that key (six entries at R = 0) before the leader's step T - 1 reads one of them: only the value
    logged at the first store of a row is the serial chain's."""
    cfg = dict(n_time_states=6, n_temp_states=2, n_balance_states=2, n_p2p_states=2)
    D, safe = _check(_shared_key_day(20), R, "f64", [0.1] * 6, **cfg)
    assert (D, safe) == (20, True)


# ------------------------------------------------------------- 2. the smallest interleaving horizon
@pytest.mark.parametrize("T,q", [(12, "f64"), (24, "f32")])
def test_smallest_horizon(T, q):
    """T = 12: L = 6, two loop iterations per phase; T = 24 with an f32 table (16-B rows and log slots)."""
    D, safe = _check(_inputs(S, N, T), 1, q, _schedule(2, 6))
    assert safe and D + 4 <= T // 2, D


# ------------------------------------------- 3. per-agent setpoints and sigma across two calls
@pytest.mark.parametrize("change", ["thermal", "sigma"])
def test_setpoints_and_sigma_across_two_calls(change):
    """Two consecutive run_episodes calls (3 + 3 episodes, the first announcing the second's epsilons)
    with per-agent setpoints and sigma = 0.45; between the calls either the setpoints or sigma change.
    Every T0 (the resets inside both chains and the one each chain leaves) must be the oracle's for
    the setpoint and sigma in force when its episode ended."""
    T, R, e0 = 24, 1, 2
    inp = _inputs(S, N, T)
    rs = np.random.RandomState(77)
    sp1 = rs.choice(SETPOINTS, (S, N))
    sp2 = sp1 if change == "sigma" else rs.choice(SETPOINTS, (S, N))
    sg1, sg2 = 0.45, (0.2 if change == "sigma" else 0.45)
    eps1, eps2 = _schedule(e0, 3), _schedule(e0 + 3, 3)

    ob = _oracle(inp, R, "f64", setpoint=sp1)
    w1, _ = _oracle_run(ob, e0, eps1, sg1)
    ob.params = dataclasses.replace(ob.params, setpoint=sp2)
    w2, out = _oracle_run(ob, e0 + 3, eps2, sg2)

    single, chain = _engine(inp, N, R), _engine(inp, N, R)
    for eng in (single, chain):
        eng.set_thermal(sp1)
    s1 = _singles(single, e0, eps1, sg1)
    chain.run_episodes(e0, eps1, reset_sigma=sg1, next_epsilons=eps2, record=WIDE)
    assert chain.last_kernel().endswith(",interleaved>"), chain.last_kernel()
    c1 = chain.episode_rewards()
    assert np.array_equal(c1, s1) and np.array_equal(c1, w1)
    if change == "thermal":
        for eng in (single, chain):
            eng.set_thermal(sp2)
    s2 = _singles(single, e0 + 3, eps2, sg2)
    c2 = _chain(chain, e0 + 3, eps2, sg2)
    assert np.array_equal(c2, s2) and np.array_equal(c2, w2)
    _same(chain, single, ob, out, "f64")
    single.close()
    chain.close()


# ------------------------------------------------------------------------- 4. the 64 + 6 split
def test_70_episode_call():
    """70 episodes at T = 12 run as two launches (64 + 6): the T0 the first leaves is the one the second
    starts from, and each launch's log starts empty."""
    _check(_inputs(S, N, 12), 1, "f64", _schedule(0, 70), e0=0)
