"""The object API's day profiles on the device's own runs: CommunityMicrogrid.day_profile() after run(),
tabular and rule, and run_days(days, profile=True), against the reference helper (tests/day_profile_ref.py)
applied to the run's records and to the oracle's episode of the same days."""
import numpy as np
import pytest

import day_profile_ref as ref
import summary_cases
from test_gpu_summary import _tabular_community

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.mark.parametrize("kind", ["tabular", "rule"])
def test_community_day_profile_after_run(kind):
    from oracle.restatement import OracleParams
    from p2pmicrogrid_amd import community
    from p2pmicrogrid_amd.day_profile import as_dict
    from p2pmicrogrid_amd.environment import env
    N = 2
    if kind == "rule":
        np.random.seed(42)
        com = community.get_rule_based_community(N, homogeneous=False)
    else:
        com, _ = _tabular_community(N)
    com.agents[0].heating.set_state(19.0, 19.0)
    with pytest.raises(RuntimeError):
        com.day_profile()
    T = len(env)
    load = np.stack([a.load_series(T) for a in com.agents])[None]
    pv = np.stack([a.pv.series(T) for a in com.agents])[None]
    power, cost = com.run()
    rec = com._engine.get_records(("cost", "grid", "p2p", "t_in", "action"))
    levels = np.broadcast_to(OracleParams().hp_levels, (1, N, 3))
    for period in (None, 8, 7):
        want = as_dict(*ref.profile(rec, levels, load, pv, F32(20.0), F32(22.0), reward=False, period=period))
        got = com.day_profile(period=period)
        assert list(got) == ["agent", "community"]
        for part in want:
            assert list(got[part]) == list(want[part])
            for k in want[part]:
                assert got[part][k].shape == want[part][k].shape[1:], (part, k)
                assert np.array_equal(got[part][k], want[part][k][0], equal_nan=True), (part, k, period)
    whole = com.day_profile()
    assert whole["agent"]["t_in"].shape == (T, N) and np.all(whole["agent"]["samples"] == 1)
    # one sample per row: the record itself, up to half a fixed-point step
    assert np.allclose(whole["agent"]["cost"], np.asarray(cost, np.float64), rtol=0, atol=2.0 ** -29)
    assert np.allclose(whole["agent"]["net_grid"] + whole["agent"]["net_p2p"], np.asarray(power, np.float64), rtol=0, atol=0.01)
    assert np.array_equal(whole["agent"]["t_in"], np.asarray(rec["t_in"][:, 0], np.float64))  # temperatures convert exactly
    assert (whole["agent"]["discomfort"] > 0).any() and (whole["agent"]["hp"] > 0).any()
    if kind == "rule":
        assert np.all(whole["agent"]["action1"] == 0) and np.all(whole["agent"]["reward"] == 0)
    kwh = com.day_profile(kwh=True)
    assert np.allclose(kwh["agent"]["load"], whole["agent"]["load"] * (15.0 / 60.0 * 1e-3), rtol=1e-15, atol=0)
    assert np.array_equal(kwh["agent"]["grid_max"], whole["agent"]["grid_max"]) and np.array_equal(kwh["agent"]["cost"], whole["agent"]["cost"])
    com._engine.close()


def test_run_days_profile():
    import role_tables
    from oracle.restatement import OracleParams
    from p2pmicrogrid_amd.day_profile import as_dict
    N, D, T = 2, 3, 96
    com, tables = _tabular_community(N)
    inp = summary_cases.batch_inputs(D, N, T, seed=31)
    inp.max_in = np.broadcast_to(np.array([F32(a.max_in) for a in com.agents], F32), (D, N)).copy()
    days = [{"time": inp.time, "t_out": inp.t_out[d], "load": inp.load_w[d], "pv": inp.pv_w[d], "t_in": inp.t_in0[d],
             "t_m": inp.t_m0[d]} for d in range(D)]
    plain = com.run_days(days)
    res, mean_day = com.run_days(days, profile=True)
    assert len(res) == D and all(sorted(r) == sorted(p) and all(np.array_equal(r[k], p[k]) for k in p) for r, p in zip(res, plain))
    # run_days returns power = grid + p2p, not the two flows, so the expected arrays come from the oracle's episode
    # of the same days, whose costs and temperatures are the per-day records' bit for bit
    out = role_tables.frozen_oracle(inp, N, com._rounds, tables).run_episode("greedy")
    assert all(np.array_equal(out["cost"][:, d], res[d]["cost"]) and np.array_equal(out["t_in"][:, d], res[d]["t_in"])
               for d in range(D))
    levels = np.broadcast_to(OracleParams().hp_levels, (D, N, 3))
    for period in (None, 4):
        want = as_dict(*ref.profile(out, levels, inp.load_w, inp.pv_w, F32(20.0), F32(22.0), reward=False, period=period))
        got = mean_day if period is None else com.run_days(days, profile=True, period=period)[1]
        for part in want:
            for k in want[part]:
                assert got[part][k].shape == want[part][k].shape[1:], (part, k)
                assert np.array_equal(got[part][k], want[part][k][0], equal_nan=True), (part, k, period)
    assert mean_day["agent"]["samples"].shape == (T, N) and np.all(mean_day["agent"]["samples"] == D)
    assert np.array_equal(mean_day["agent"]["cost"], sum(ref.fix(r["cost"], 28) for r in res) * 2.0 ** -28 / D)
    assert com.run_days([], profile=True) == ([], None)
