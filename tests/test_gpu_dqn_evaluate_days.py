"""CommunityMicrogrid.evaluate_days / load_and_run_batched for DQN communities: every evaluation day in one
greedy launch on a policy set of the agents' networks (dqn_greedy_episode_kernel), against run() day by day
(T act launches per day) from the same inputs, bit for bit: results, summaries, DB rows and np.random
consumption.  No training is run: the networks are seeded, scaled weights written into the agents."""
import numpy as np
import pytest

import dqn_eval_cases as dc
import summary_cases

pytestmark = pytest.mark.gpu
F32 = np.float32
KEYS = ("power", "cost", "decisions", "t_in", "t_in_final", "t_m_final")


def _dqn_community(n_agents, seed=7, scale=8.0):
    from p2pmicrogrid_amd import community
    from p2pmicrogrid_amd.agent import DQNAgent
    np.random.seed(42)
    com = community.get_community(DQNAgent, n_agents)
    for a, th in zip(com.agents, dc.weights(n_agents, seed, scale)):
        a.actor.q_network.set_flat_weights(th)
    return com


def _days(com, D, T, seed=31):
    N = len(com.agents)
    inp = summary_cases.batch_inputs(D, N, T, seed=seed)
    return [{"time": inp.time, "t_out": inp.t_out[d], "load": inp.load_w[d], "pv": inp.pv_w[d], "t_in": inp.t_in0[d],
             "t_m": inp.t_m0[d]} for d in range(D)]


def _run_day(com, day):
    """run() from one day's inputs: (the evaluate_days entry of that day, the engine's summary per agent)."""
    from p2pmicrogrid_amd.dataset import ProfileDataset
    from p2pmicrogrid_amd.environment import env
    ds = lambda x: ProfileDataset(np.asarray(x, F32), np.roll(np.asarray(x, F32), -1, 0))  # noqa: E731
    env.setup(ds(np.stack([day["time"], day["t_out"]], axis=1)))
    for i, a in enumerate(com.agents):
        a.set_profiles(ds(day["load"][i]), ds(day["pv"][i]))
        a.heating.set_state(day["t_in"][i], day["t_m"][i])
    power, cost = com.run()
    t_in, t_m = com._engine.get_temperatures()
    out = {"power": power, "cost": cost, "decisions": com.decisions.copy(),
           "t_in": com._engine.get_record("t_in")[:, 0, :], "t_in_final": t_in[0], "t_m_final": t_m[0]}
    return out, com.summary()


def _same_day(got, want, tag):
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (tag, k)
        assert np.array_equal(got[k], want[k]), (tag, k)


def test_evaluate_days_equals_run_day_by_day():
    from p2pmicrogrid_amd.day_profile import as_dict, from_records
    from p2pmicrogrid_amd.community import thermal_arrays
    N, D, T = 2, 3, 12
    com = _dqn_community(N)
    days = _days(com, D, T)
    plain = com.evaluate_days(days)
    assert len(plain) == D and all(sorted(r) == sorted(KEYS) for r in plain)
    res = com.evaluate_days(days, summary=True)
    res_p, mean_day = com.evaluate_days(days, profile=True, period=4)
    seen = set()
    for d, day in enumerate(days):
        want, totals = _run_day(com, day)
        _same_day(plain[d], want, d)
        _same_day(res[d], want, d)
        _same_day(res_p[d], want, d)
        assert sorted(res[d]) == sorted(KEYS + ("summary",)) and list(res[d]["summary"]) == list(totals)
        for k in totals:
            assert res[d]["summary"][k].shape == (N,) and np.array_equal(res[d]["summary"][k], totals[k]), (d, k)
        seen |= {float(x) for x in np.unique(want["decisions"])}
    assert len(seen) == 3, seen  # off, half and full power occur: the policy is not constant
    # the mean day: day_profile.from_records on the records evaluate_days returns (power = grid + p2p is not a
    # record, so the flows come from a batch of the same days)
    from p2pmicrogrid_amd.dqn import DeviceDQNBatch
    from p2pmicrogrid_amd.engine import price_table
    levels, params = thermal_arrays(com.agents)
    load, pv = (np.stack([np.asarray(d[k], F32) for d in days]) for k in ("load", "pv"))
    time_f, t_out = (np.stack([np.asarray(d[k], F32) for d in days]) for k in ("time", "t_out"))
    eng = DeviceDQNBatch(D, N, com._rounds, T, capacity=32, init_seed=None)
    eng.set_weights("online", np.tile(np.stack([a.actor.q_network.flat_weights() for a in com.agents]), (D, 1)))
    eng.set_env(time_f, t_out, *price_table(time_f))
    eng.set_profiles(load, pv)
    eng.set_max_in(np.broadcast_to(np.array([F32(a.max_in) for a in com.agents], F32), (D, N)))
    eng.set_temperatures(np.stack([d["t_in"] for d in days]), np.stack([d["t_m"] for d in days]))
    rec = ("grid", "p2p", "cost", "t_in", "action")
    eng.run_episode("greedy", record=rec)
    r = eng.get_records(rec)
    eng.close()
    assert all(np.array_equal(r["cost"][:, d], plain[d]["cost"]) for d in range(D))
    par = np.broadcast_to(params, (D, N, 4))
    want = as_dict(*from_records(r, np.broadcast_to(levels, (D, N, 3)), load, pv, par[..., 1], par[..., 2], period=4))
    for part in want:
        assert list(mean_day[part]) == list(want[part])
        for k in want[part]:
            assert np.array_equal(mean_day[part][k], want[part][k][0], equal_nan=True), (part, k)
    assert com.evaluate_days([]) == [] and com.evaluate_days([], profile=True) == ([], None)
    com._engine.close()


def test_tabular_communities_delegate_to_run_days():
    from test_gpu_summary import _tabular_community
    com, _ = _tabular_community(2)
    days = _days(com, 2, 12)
    a, b = com.evaluate_days(days, summary=True), com.run_days(days, summary=True)
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k in KEYS:
            assert np.array_equal(x[k], y[k]), k
        assert all(np.array_equal(x["summary"][k], y["summary"][k]) for k in y["summary"])


def test_rule_communities_are_refused():
    from p2pmicrogrid_amd import community
    np.random.seed(1)
    with pytest.raises(NotImplementedError):
        community.get_rule_based_community(2, False).evaluate_days([{}])


def test_batched_dqn_evaluation_equals_day_by_day(tmp_path, monkeypatch):
    from p2pmicrogrid_amd import community, database as db, rl, setup
    monkeypatch.setattr(rl, "MODELS_DIR", str(tmp_path))
    monkeypatch.setattr(setup, "implementation", "dqn")
    setting = community.setting_name()
    com = _dqn_community(setup.nr_agents)
    for a in com.agents:
        a.save_to_file(setting, "dqn")  # seeded weights, no training
    runs = []
    for k, fn in enumerate((community.load_and_run, community.load_and_run_batched)):
        con = db.get_connection(str(tmp_path / f"results{k}.db"))
        db.create_tables(con.cursor())
        np.random.seed(7)
        out = fn(con, is_testing=True)
        runs.append((out, db.get_test_results(con), db.get_rounds_decisions(con), np.random.get_state()))
    (a, res_a, rd_a, st_a), (b, res_b, rd_b, st_b) = runs
    assert sorted(a) == sorted(b) and len(a) == 5
    for day in a:
        for k in ("power", "cost", "decisions"):
            assert a[day][k].shape == b[day][k].shape and a[day][k].dtype == b[day][k].dtype, (day, k)
            assert np.array_equal(a[day][k], b[day][k]), (day, k)
    levels = {float(x) for v in a.values() for x in np.unique(v["decisions"])}
    assert len(levels) == 3, levels  # the seeded networks use all three heat-pump levels
    assert len(res_a) == 96 * setup.nr_agents * 5 and res_a.equals(res_b)
    assert len(rd_a) == 96 * setup.nr_agents * 5 * (setup.rounds + 1) and rd_a.equals(rd_b)
    # the same draws were taken from np.random, in the same order
    assert st_a[0] == st_b[0] and np.array_equal(st_a[1], st_b[1]) and st_a[2:] == st_b[2:]
