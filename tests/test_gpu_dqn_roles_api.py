"""CommunityMicrogrid.train_days: one DQN community of N agents trained over D days at once on a role engine
(DeviceDQNBatch(shared="role")), against the same engine driven by hand from the same inputs, weights and calls,
and the trained networks as evaluate_days and run() then see them.  T = 32: one fill episode admits training."""
import numpy as np
import pytest

from test_gpu_dqn_evaluate_days import _days, _dqn_community, _run_day, _same_day

pytestmark = pytest.mark.gpu
F32 = np.float32
N, D, T = 2, 3, 32
STATE = ("online", "target", "adam_m", "adam_v")


def _hand_engine(com, days):
    """The role engine train_days builds, from the community's current values."""
    from p2pmicrogrid_amd.community import dqn_learning_arrays, thermal_arrays
    from p2pmicrogrid_amd.dqn import DeviceDQNBatch
    from p2pmicrogrid_amd.engine import price_table
    stack = lambda k: np.stack([np.asarray(d[k], F32) for d in days])  # noqa: E731
    eng = DeviceDQNBatch(D, N, com._rounds, T, shared="role", capacity=com.agents[0].trainer.buffer.buffer_size,
                         init_seed=None)
    time_f = stack("time")
    eng.set_env(time_f, stack("t_out"), *price_table(time_f))
    eng.set_profiles(stack("load"), stack("pv"))
    eng.set_max_in(np.broadcast_to(np.array([F32(a.max_in) for a in com.agents], F32), (D, N)))
    levels, params = thermal_arrays(com.agents)
    eng.set_hp_levels(np.broadcast_to(levels, (D, N, 3)))
    par = np.broadcast_to(params, (D, N, 4))
    eng.set_thermal(par[..., 0], cop=par[..., 3], lower=par[..., 1], upper=par[..., 2])
    eng.set_weights("online", np.stack([a.actor.q_network.flat_weights() for a in com.agents]))
    eng.set_weights("target", np.stack([a.trainer.target_network.flat_weights() for a in com.agents]))
    gamma, tau, lr = dqn_learning_arrays(com.agents)
    eng.set_learning(gamma=gamma, tau=tau, lr=lr)
    return eng, stack("t_in"), stack("t_m")


def _hand_episode(eng, t_in, t_m, mode, episode, eps):
    eng.set_temperatures(t_in, t_m)
    eng.run_episode(mode, "philox", episode=episode, epsilon=eps, record=("loss",) if mode == "train" else ())
    if mode == "train":
        return (float(np.mean(eng.episode_reward(), dtype=np.float32)), float(np.mean(eng.get_record("loss"), dtype=np.float32)))


def test_train_days_equals_the_role_engine_driven_by_hand():
    com = _dqn_community(N, scale=1.0)
    for a in com.agents:  # a learning rate at which 64 Adam steps show in the greedy policy's Q values
        a.trainer.optimizer.learning_rate = 1e-3
    com.agents[1].trainer._tau = 0.05
    days = _days(com, D, T)
    eps = float(com.agents[0].actor._epsilon)
    start = np.stack([a.actor.q_network.flat_weights() for a in com.agents])
    hand, t_in, t_m = _hand_engine(com, days)
    want = [_hand_episode(hand, t_in, t_m, mode, ep, eps) for ep, mode in enumerate(("fill", "train", "train"))][1:]
    got = com.train_days(days, episodes=2, fill=1)
    assert got == want and len(got) == 2 and all(np.isfinite(x) for pair in got for x in pair)
    assert com._engine is None  # no community engine was needed
    online = np.stack([a.actor.q_network.flat_weights() for a in com.agents])
    target = np.stack([a.trainer.target_network.flat_weights() for a in com.agents])
    assert np.array_equal(online, hand.get_weights("online")) and np.array_equal(target, hand.get_weights("target"))
    assert not np.array_equal(online, start) and not np.array_equal(online[0], online[1])
    assert list(hand.net_steps()) == [2 * T] * N
    # the trained networks are what evaluate_days and run() use, and run()'s engine takes over the Adam state
    res = com.evaluate_days(days)
    day0, _ = _run_day(com, days[0])
    _same_day(res[0], day0, "day 0")
    ceng = com._engine
    assert np.array_equal(ceng.get_weights("online"), online)
    assert np.array_equal(ceng.get_weights("adam_m"), hand.get_weights("adam_m"))
    assert np.array_equal(ceng.get_weights("adam_v"), hand.get_weights("adam_v"))
    assert list(ceng.net_steps()) == [2 * T] * N
    assert np.array_equal(ceng.get_learning()["tau"].reshape(-1), [0.005, 0.05])
    # a second call: the kept engine (its rings stay, no new fill), the Adam state read from the community engine
    want2 = _hand_episode(hand, t_in, t_m, "train", 3, eps)
    role = com._role[1]
    got2 = com.train_days(days, episodes=1)
    assert com._role[1] is role and got2 == [want2]
    for k in STATE:
        assert np.array_equal(role.get_weights(k), hand.get_weights(k)), k
    assert np.array_equal(ceng.get_weights("online"), hand.get_weights("online"))
    assert np.array_equal(ceng.get_weights("target"), hand.get_weights("target"))
    assert np.array_equal(ceng.get_weights("adam_v"), hand.get_weights("adam_v"))
    assert list(ceng.net_steps()) == [3 * T] * N
    buf_a, added_a = role.get_buffer()
    buf_b, added_b = hand.get_buffer()
    assert np.array_equal(added_a, added_b) and list(added_a) == [4 * T] * (D * N)
    assert np.array_equal(buf_a[:, :4 * T], buf_b[:, :4 * T])
    hand.close()
    role.close()
    ceng.close()


def test_tabular_and_rule_communities_raise():
    from p2pmicrogrid_amd import community
    from test_gpu_summary import _tabular_community
    com, _ = _tabular_community(2)
    with pytest.raises(TypeError, match="role"):
        com.train_days(_days(com, 2, 12))
    np.random.seed(1)
    with pytest.raises(TypeError, match="nothing to train"):
        community.get_rule_based_community(2, False).train_days([{}])
