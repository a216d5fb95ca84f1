"""CommunityMicrogrid.evaluate_policies: K policy snapshots x D days in one launch of policy_episode_kernel,
against evaluate_days run when the agents held each snapshot's tables, and a DQN community's discretised policy
(ActorModel.policy_map bytes on the default grid) against the oracle holding the one-hot tables of those bytes:
the byte-order contract between p2pmg_dqn_policy_map and the tabular rows."""
import numpy as np
import pytest

import policy_set_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32


def test_snapshots_times_days_equal_evaluate_days_per_snapshot():
    from p2pmicrogrid_amd import community
    from p2pmicrogrid_amd.agent import QAgent
    K, D, N, T = 3, 4, 2, 12
    np.random.seed(42)
    com = community.get_community(QAgent, N)
    days = ref.days_of(ref.day_inputs(com, D, T))
    snaps, want = [], []
    for k in range(K):  # after 0, 1 and 2 training episodes
        if k:
            com.train_episode()
        snaps.append(np.stack([a.actor.policy_bytes() for a in com.agents]))
        assert np.array_equal(snaps[-1], np.stack([a.actor.greedy_policy().reshape(-1) for a in com.agents]))
        want.append(com.evaluate_days(days, summary=True))
    snaps = np.stack(snaps)
    assert snaps.shape == (K, N, 160000) and np.all(snaps[0] == 255) and (snaps[1] != 255).any()
    assert not np.array_equal(snaps[1], snaps[2])
    plain = com.evaluate_policies(days, snaps)
    res = com.evaluate_policies(days, snaps.reshape(K, N, 20, 20, 20, 20), summary=True)
    res_p, prof = com.evaluate_policies(days, snaps, profile=True, period=4)
    assert len(plain) == len(res) == len(res_p) == K
    for k in range(K):
        assert len(plain[k]) == D and all(sorted(r) == sorted(ref.DAY_KEYS) for r in plain[k])
        for d in range(D):
            for got in (plain[k][d], res[k][d], res_p[k][d]):
                ref.assert_same_day(got, want[k][d], (k, d))
            assert list(res[k][d]["summary"]) == list(want[k][d]["summary"])
            for name, v in want[k][d]["summary"].items():
                assert np.array_equal(res[k][d]["summary"][name], v), (k, d, name)
    # the profile's groups are the snapshot indices: row k is run_days' mean day under snapshot k's tables
    assert prof["agent"]["cost"].shape == (K, 4, N) and prof["community"]["samples"].shape == (K, 4)
    assert np.all(prof["agent"]["samples"] == D * T // 4)
    for k in range(K):
        for a, t in zip(com.agents, snaps[k]):  # the agents hold snapshot k's policy again, as one-hot tables
            a.actor.set_qtable(ref.one_hot_tables(t[None], dtype=np.float64)[0].reshape(20, 20, 20, 20, 3))
        _, mean_day = com.run_days(days, profile=True, period=4)
        for part in mean_day:
            for name, v in mean_day[part].items():
                assert np.array_equal(prof[part][name][k], v, equal_nan=True), (k, part, name)
    assert com.evaluate_policies([], snaps) == [] and com.evaluate_policies(days, snaps[:0], profile=True) == ([], None)
    with pytest.raises(ValueError, match="uint8"):
        com.evaluate_policies(days, snaps.astype(np.int32))
    if com._engine is not None:
        com._engine.close()


def test_dqn_policy_maps_cost_what_the_oracle_says():
    """A DQN community trained for one episode over two days (train_days), its policy maps on the default grid
    fed to evaluate_policies: the result is the oracle's greedy run on the one-hot tables of those bytes."""
    from p2pmicrogrid_amd.community import ACTION_LEVELS, thermal_arrays
    N, D, T = 2, 3, 12
    com = ref.dqn_community(N)
    com.train_days(ref.days_of(ref.day_inputs(com, 2, 32, seed=5)), episodes=1, fill=1)
    maps = com.policy_maps()
    assert maps.shape == (N, 20, 20, 20, 20) and maps.dtype == np.uint8 and maps.max() <= 2 and len(np.unique(maps)) > 1
    inp = ref.day_inputs(com, D, T)
    days = ref.days_of(inp)
    got = com.evaluate_policies(days, maps[None])
    assert len(got) == 1 and len(got[0]) == D
    levels, params = thermal_arrays(com.agents)
    th = (np.broadcast_to(params[:, 0].astype(np.float64), (D, N)), np.broadcast_to(params[:, 3].astype(np.float64), (D, N)),
          np.broadcast_to(levels, (D, N, 3)))
    out = ref.oracle_policy_run(inp, N, com._rounds, maps.reshape(N, -1), np.arange(D * N) % N, thermal=th)
    max_power = np.array([a.heating.hp.max_power for a in com.agents])
    seen = set()
    for d in range(D):
        g = got[0][d]
        assert np.array_equal(g["cost"], out["cost"][:, d]) and np.array_equal(g["t_in"], out["t_in"][:, d]), d
        assert np.array_equal(g["power"], (out["grid"][:, d] + out["p2p"][:, d]).astype(F32)), d
        assert np.array_equal(g["decisions"], np.array(ACTION_LEVELS)[out["action"][:, :, d]] * max_power[None, None, :]), d
        assert np.array_equal(g["t_in_final"], out["t_in_final"][d]) and np.array_equal(g["t_m_final"], out["t_m_final"][d])
        seen |= set(np.unique(out["action"][:, :, d]))
    assert len(seen) > 1, seen  # the discretised policy is not constant on these days
    # ... and it is the policy, not the grid order, that the episode read: the actions are the map's bytes at the rows
    it, iT, ib, ip = (out["idx"][..., j] for j in range(4))
    row = ((it * 20 + iT) * 20 + ib) * 20 + ip
    role = np.broadcast_to(np.arange(N), row.shape)
    assert np.array_equal(out["action"], maps.reshape(N, -1)[role, row])
    role = getattr(com, "_role", None)
    for e in (com._engine, role[1] if role else None):
        if e is not None:
            e.close()
