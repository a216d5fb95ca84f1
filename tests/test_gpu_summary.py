"""p2pmg_episode_summary on the device: both arrays bit for bit the NumPy definition
(tests/summary_ref.py) applied to the ORACLE's episode, for every kernel and record layout a launch
can leave (tests/summary_cases.py), plus the error states, chained launches and the object API."""
import numpy as np
import pytest

import summary_cases
import summary_ref
from summary_cases import CASES, RECORDS

pytestmark = pytest.mark.gpu
F32 = np.float32


def _device(c, inp):
    from p2pmicrogrid_amd.engine import DeviceCommunityBatch
    if c.kind == "dqn":
        from oracle import dqn as odqn
        from p2pmicrogrid_amd.dqn import DeviceDQNBatch
        eng = DeviceDQNBatch(c.S, c.N, c.R, c.T, init_seed=None)
        th = odqn.glorot_init(c.S * c.N, summary_cases.DQN_INIT_SEED)
        eng.set_weights("online", th)
        eng.set_weights("target", th)
    else:
        eng = DeviceCommunityBatch(c.S, c.N, c.R, c.T, q_dtype=c.q_dtype, shared_q=c.shared)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    if c.tables() is not None:
        eng.set_q(c.tables())
    if c.hp_levels() is not None:
        eng.set_hp_levels(c.hp_levels())
    if c.setpoints is not None:
        eng.set_thermal(c.setpoint())
    if c.battery:
        eng.set_battery(c.battery_capacity(), 0.1, 0.9, 0.9)
    return eng


def _launch(c, inp, eng, record=RECORDS):
    if c.kind == "rule":
        t0, on = c.rule_state()
        eng.set_temperatures(t0, t0)
        eng.set_hp_state(on.astype(F32))
        eng.run_rule_episode(record=[r for r in record if r != "reward"])
    elif c.kind == "dqn":
        eng.run_episode("fill", "philox", episode=0, epsilon=1.0)
        eng.set_temperatures(inp.t_in0, inp.t_m0)
        eng.run_episode("greedy", record=record)
    elif c.mode == "train":
        eng.run_episode("train", "philox", episode=c.episode, epsilon=c.eps, record=record, kernel=c.kernel)
    else:
        eng.run_episode("greedy", record=record, kernel=c.kernel)


def _arrays(summary):
    """episode_summary()'s dict as ([S, N, 16], [S, 16]) in field order."""
    return (np.stack([summary["agent"][n] for n in summary_ref.FIELDS], axis=-1),
            np.stack([summary["scenario"][n] for n in summary_ref.FIELDS], axis=-1))


def _assert_equal(got, want, tag):
    for g, w, what in zip(got, want, ("agent", "scenario")):
        assert g.shape == w.shape and g.dtype == np.float64, (tag, what)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            k = tuple(bad[0])
            raise AssertionError(f"{tag} {what}: {len(bad)} of {g.size} differ, first at {k} "
                                 f"(field {summary_ref.FIELDS[k[-1]]}): {g[k]!r} != {w[k]!r}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_summary_matches_oracle(name):
    e = summary_cases.expected(name)
    c, inp = e["case"], e["inp"]
    eng = _device(c, inp)
    _launch(c, inp, eng)
    assert c.last_kernel in eng.last_kernel(), eng.last_kernel()
    if name.startswith("fast"):
        assert eng.last_kernel().startswith("episode_fast_kernel")
    got = _arrays(eng.episode_summary())
    _assert_equal(got, (e["agent"], e["scenario"]), name)
    if c.kind == "rule":
        assert np.all(got[0][..., 1] == 0)
    eng.close()


@pytest.mark.parametrize("name", ["fast_train", "general", "sq16_many", "rule"])
def test_summary_equals_helper_on_the_launch_own_records(name):
    """Consistency: the device's summary against the helper applied to what get_records returns from
    the same launch (both layouts), and either output pointer alone."""
    from p2pmicrogrid_amd import _lib
    e = summary_cases.expected(name)
    c, inp = e["case"], e["inp"]
    eng = _device(c, inp)
    _launch(c, inp, eng)
    rec = eng.get_records([r for r in RECORDS if not (c.kind == "rule" and r == "reward")])
    lower, upper = c.bounds()
    want = summary_ref.summary(rec, eng.get_hp_levels(), inp.load_w, inp.pv_w, lower, upper, reward="reward" in rec)
    th = eng.get_thermal()
    assert np.array_equal(th[..., 1], lower) and np.array_equal(th[..., 2], upper)
    _assert_equal(_arrays(eng.episode_summary()), want, name)
    ag = np.full((eng.A, 16), np.nan)
    sc = np.full((eng.S, 16), np.nan)
    assert eng.L.p2pmg_episode_summary(eng._ctx, ag.ctypes.data, None) == _lib.P2PMG_OK
    assert eng.L.p2pmg_episode_summary(eng._ctx, None, sc.ctypes.data) == _lib.P2PMG_OK
    _assert_equal((ag.reshape(eng.S, eng.N, 16), sc), want, name + " single pointer")
    assert eng.L.p2pmg_episode_summary(eng._ctx, None, None) == 1  # P2PMG_E_INVALID
    eng.close()


def test_kwh_scales_the_energy_fields_only():
    e = summary_cases.expected("fast_greedy")
    eng = _device(e["case"], e["inp"])
    _launch(e["case"], e["inp"], eng)
    w, k = _arrays(eng.episode_summary()), _arrays(eng.episode_summary(kwh=True))
    scale = np.ones(16)
    scale[2:10] = 15.0 / 60.0 * 1e-3
    for a, b in zip(w, k):
        assert np.array_equal(b, a * scale)
    eng.close()


@pytest.mark.parametrize("name", ["fast_greedy", "general"])
def test_missing_records_are_a_state_error_that_names_them(name):
    from p2pmicrogrid_amd._lib import P2PMGError
    e = summary_cases.expected(name)
    c, inp = e["case"], e["inp"]
    eng = _device(c, inp)
    with pytest.raises(P2PMGError, match=r"STATE.*no episode has run.*cost"):
        eng.episode_summary()
    _launch(c, inp, eng, record=("reward", "cost"))  # fast kernel: the narrow rows
    with pytest.raises(P2PMGError, match=r"STATE.*did not record grid, p2p, t_in, action"):
        eng.episode_summary()
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    _launch(c, inp, eng, record=("reward", "cost", "grid", "p2p", "t_in"))
    with pytest.raises(P2PMGError, match=r"STATE.*did not record action$"):
        eng.episode_summary()
    # a full launch afterwards is summarised as if nothing had happened before
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    _launch(c, inp, eng)
    _assert_equal(_arrays(eng.episode_summary()), (e["agent"], e["scenario"]), name)
    # without the reward record field 1 is 0, everything else as before
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    _launch(c, inp, eng, record=[r for r in RECORDS if r != "reward"])
    ag, sc = _arrays(eng.episode_summary())
    assert np.all(ag[..., 1] == 0) and np.all(sc[:, 1] == 0)
    assert np.array_equal(np.delete(ag, 1, -1), np.delete(e["agent"], 1, -1))
    assert np.array_equal(np.delete(sc, 1, -1), np.delete(e["scenario"], 1, -1))
    eng.close()


def test_after_a_chain_the_summary_is_the_last_episodes():
    """run_episodes of 3 chained episodes with full records == the third episode launched alone."""
    c = CASES["fast_train"]
    inp = c.inputs()
    eps = [0.8, 0.7, 0.6]
    a = _device(c, inp)
    a.run_episodes(0, eps, reset_sigma=0.3, record=RECORDS)
    assert a.last_kernel().startswith("episode_fast_kernel")
    b = _device(c, inp)
    b.run_episodes(0, eps[:2], reset_sigma=0.3, next_epsilons=eps[2:])
    b.run_episode("train", "philox", episode=2, epsilon=eps[2], record=RECORDS, reset_sigma=0.3)
    got, want = _arrays(a.episode_summary()), _arrays(b.episode_summary())
    _assert_equal(got, want, "chain")
    rec = a.get_records(RECORDS)
    lower, upper = c.bounds()
    _assert_equal(got, summary_ref.summary(rec, a.get_hp_levels(), inp.load_w, inp.pv_w, lower, upper), "chain records")
    assert not np.array_equal(got[0], summary_cases.expected("fast_train")["agent"])  # not episode 0's
    a.close()
    b.close()


def _seq_sum64(col):
    acc = np.zeros(col.shape[1:], np.float64)
    for t in range(col.shape[0]):
        acc = acc + col[t].astype(np.float64)
    return acc


def _tabular_community(n_agents, seed=42):
    from p2pmicrogrid_amd import community
    import role_tables
    np.random.seed(seed)
    com = community.get_rl_based_community(n_agents, homogeneous=False)
    tables = role_tables.random_tables(n_agents, seed=9)
    for a, t in zip(com.agents, tables):
        a.actor.set_qtable(t.reshape(20, 20, 20, 20, 3))
    return com, tables


def test_run_days_summary():
    from oracle.restatement import OracleParams
    import role_tables
    N, D, T = 2, 3, 96
    com, tables = _tabular_community(N)
    inp = summary_cases.batch_inputs(D, N, T, seed=31)
    inp.max_in = np.broadcast_to(np.array([F32(a.max_in) for a in com.agents], F32), (D, N)).copy()
    days = [{"time": inp.time, "t_out": inp.t_out[d], "load": inp.load_w[d], "pv": inp.pv_w[d], "t_in": inp.t_in0[d],
             "t_m": inp.t_m0[d]} for d in range(D)]
    plain = com.run_days(days)
    assert all(sorted(r) == ["cost", "decisions", "power", "t_in", "t_in_final", "t_m_final"] for r in plain)
    res = com.run_days(days, summary=True)
    out = role_tables.frozen_oracle(inp, N, com._rounds, tables).run_episode("greedy")
    want, _ = summary_ref.summary(out, np.broadcast_to(OracleParams().hp_levels, (D, N, 3)), inp.load_w, inp.pv_w,
                                  F32(20.0), F32(22.0), reward=False)  # run_days, like run(), records no reward
    for d, (r, p) in enumerate(zip(res, plain)):
        assert sorted(r) == sorted(list(p) + ["summary"])
        assert all(np.array_equal(r[k], p[k]) for k in p)
        assert list(r["summary"]) == list(summary_ref.FIELDS)
        assert np.array_equal(r["summary"]["cost"], _seq_sum64(r["cost"])), d
        for k, n in enumerate(summary_ref.FIELDS):
            assert r["summary"][n].shape == (N,) and np.array_equal(r["summary"][n], want[d, :, k]), (d, n)


@pytest.mark.parametrize("kind", ["tabular", "rule"])
def test_community_summary_after_run(kind):
    from oracle.restatement import OracleBatch, OracleParams
    from p2pmicrogrid_amd import community
    from p2pmicrogrid_amd.engine import price_table
    from p2pmicrogrid_amd.environment import env
    N = 2
    if kind == "rule":
        np.random.seed(42)
        com, tables = community.get_rule_based_community(N, homogeneous=False), None
    else:
        com, tables = _tabular_community(N)
    com.agents[0].heating.set_state(19.0, 19.0)
    T = len(env)
    time_f, t_out = env.arrays()
    load = np.stack([a.load_series(T) for a in com.agents])[None]
    pv = np.stack([a.pv.series(T) for a in com.agents])[None]
    ob = OracleBatch(S=1, N=N, R=com._rounds, load_w=load, pv_w=pv, max_in=np.array([[a.max_in for a in com.agents]]),
                     env_time=np.asarray(time_f).reshape(1, -1), env_tout=np.asarray(t_out).reshape(1, -1),
                     price_table=price_table(time_f))
    ob.t_in = np.array([[a.heating.temperature[0] for a in com.agents]], F32)
    ob.t_m = np.array([[a.heating.building_mass_temperature[0] for a in com.agents]], F32)
    if kind == "rule":
        out = ob.run_rule_episode(np.zeros((1, N), np.int64))
        out["action"] = np.where(out["on"] == 1, 2, 0)[:, None]
    else:
        ob.q[:] = tables
        out = ob.run_episode("greedy")
    with pytest.raises(RuntimeError):
        com.summary()
    power, cost = com.run()
    got = com.summary()
    want, _ = summary_ref.summary(out, np.broadcast_to(OracleParams().hp_levels, (1, N, 3)), load, pv, F32(20.0),
                                  F32(22.0), reward=False)
    assert list(got) == list(summary_ref.FIELDS)
    assert np.array_equal(got["cost"], _seq_sum64(np.asarray(cost)))
    for k, n in enumerate(summary_ref.FIELDS):
        assert got[n].shape == (N,) and np.array_equal(got[n], want[0, :, k]), n
    assert (got["discomfort_steps"] > 0).any() and (got["hp"] > 0).any()
    assert np.array_equal(com.summary(kwh=True)["load"], got["load"] * (15.0 / 60.0 * 1e-3))
    com._engine.close()
