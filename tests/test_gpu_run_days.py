"""CommunityMicrogrid.run_days / load_and_run_batched: every evaluation day in one greedy launch on
per-role tables, against the day-by-day load_and_run from the same seed, bit for bit: results, DB
rows and np.random consumption."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("homogeneous", [False, True])
def test_batched_evaluation_equals_day_by_day(tmp_path, monkeypatch, homogeneous):
    from p2pmicrogrid_amd import community, database as db, rl, setup
    monkeypatch.setattr(rl, "MODELS_DIR", str(tmp_path))
    monkeypatch.setattr(setup, "homogeneous", homogeneous)
    np.random.seed(42)
    community.main(episodes=2, verbose=False)  # trains and saves the tables both runs load
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
    assert any(np.count_nonzero(v["decisions"]) for v in a.values())  # the trained tables do heat
    assert len(res_a) == 96 * setup.nr_agents * 5 and res_a.equals(res_b)
    assert len(rd_a) == 96 * setup.nr_agents * 5 * (setup.rounds + 1) and rd_a.equals(rd_b)
    # the same draws were taken from np.random, in the same order
    assert st_a[0] == st_b[0] and np.array_equal(st_a[1], st_b[1]) and st_a[2:] == st_b[2:]


def test_run_days_needs_tabular_agents():
    from p2pmicrogrid_amd import community
    from p2pmicrogrid_amd.agent import DQNAgent
    np.random.seed(1)
    for com in (community.get_rule_based_community(2, False), community.get_community(DQNAgent, 2)):
        with pytest.raises(NotImplementedError):
            com.run_days([{}])
