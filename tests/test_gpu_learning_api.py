"""The drop-in boundary of per-agent learner constants: a community whose QActors learn at different
rates (rl.py:58-71) trains on the device like the oracle fed the same inputs and the reference's
np.random stream, and a hand-stepped QActor follows QActor.train's formula (rl.py:125-128)."""
import numpy as np
import pytest

from oracle.restatement import OracleBatch, OracleParams, reference_replay_codes

pytestmark = pytest.mark.gpu


def test_community_with_different_learning_rates_trains_like_oracle():
    from p2pmicrogrid_amd import community, setup
    from p2pmicrogrid_amd.agent import QAgent
    from p2pmicrogrid_amd.environment import env
    from p2pmicrogrid_amd.rl import QActor
    n = 2
    setup.homogeneous = True  # HPHeating reads the module flag (heating.py:101,149)
    try:
        np.random.seed(42)
        com = community.get_community(QAgent, n, homogeneous=True)
        com.agents[0].actor = QActor(20, 20, 20, 20, alpha=1e-3, gamma=0.5, epsilon=0.81)
        T, R = len(env), setup.rounds
        time_f, t_out = env.arrays()
        load = np.stack([a.load_series(T) for a in com.agents]).astype(np.float32)
        pv = np.stack([a.pv.series(T) for a in com.agents]).astype(np.float32)
        max_in = np.array([np.float32(a.max_in) for a in com.agents], np.float32)
        alphas = [np.array([[1e-3, com.agents[1].actor._alpha]]), np.array([[0.05, com.agents[1].actor._alpha]])]
        gamma = np.array([[0.5, com.agents[1].actor._gamma]])
        ob = OracleBatch(S=1, N=n, R=R, load_w=load[None], pv_w=pv[None], max_in=max_in[None],
                         env_time=np.asarray(time_f, np.float32)[None], env_tout=np.asarray(t_out, np.float32)[None])
        rs = np.random.RandomState(42)  # homogeneous: nothing drawn before the first episode
        for e in range(2):
            if e == 1:
                com.agents[0].actor._alpha = 0.05  # changed between episodes: uploaded again
            ob.params = OracleParams(alpha=alphas[e], gamma=gamma)
            ob.t_in = np.array([[a.heating.temperature[0] for a in com.agents]], np.float32)
            ob.t_m = np.array([[a.heating.building_mass_temperature[0] for a in com.agents]], np.float32)
            eps = [a.actor._epsilon for a in com.agents]
            reward, loss = com.train_episode()
            got = com._engine.get_learning()
            assert np.array_equal(got["alpha"], alphas[e]) and np.array_equal(got["gamma"], gamma)
            out = ob.run_episode("train", codes=reference_replay_codes(rs, T, R, n, eps)[:, :, None, :], eps=eps[0])
            assert loss == 0.0 and reward == float(out["episode_reward"][0]), e
            assert np.array_equal(com.last_rewards, out["reward"][:, 0, :]), e
            assert np.array_equal(com.decisions, np.array([0.0, 0.5, 1.0])[out["action"][:, :, 0, :]] * 3e3), e
            tabs = np.stack([a.actor.q_table for a in com.agents])
            assert np.array_equal(tabs.reshape(n, -1, 3), ob.q), e
            assert np.count_nonzero(tabs[0]) > 0 and np.count_nonzero(tabs[1]) > 0
    finally:
        setup.homogeneous = False


def test_hand_stepped_qactor_uses_its_own_alpha_and_gamma():
    from p2pmicrogrid_amd.rl import QActor
    a = QActor(20, 20, 20, 20, alpha=0.1, gamma=0.3)
    rs = np.random.RandomState(1)
    table = rs.uniform(-1, 1, (20, 20, 20, 20, 3))
    a.set_qtable(table)
    want = table.copy()
    for _ in range(12):
        s = np.array([rs.uniform(0, 1), *rs.uniform(-1, 1, 3)], np.float32)
        ns = np.array([rs.uniform(0, 1), *rs.uniform(-1, 1, 3)], np.float32)
        act, r = int(rs.randint(3)), np.float32(rs.uniform(-5, 0))
        a.train(s, act, r, ns)
        i, j = a._get_state_indices(s), a._get_state_indices(ns)
        want[i][act] = want[i][act] + 0.1 * ((np.float64(r) + 0.3 * np.max(want[j])) - want[i][act])
    assert np.array_equal(a.q_table, want)
    assert not np.array_equal(want, table)
