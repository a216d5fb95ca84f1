"""The object API honours each DQNAgent's own Trainer(gamma, tau, Adam(learning_rate)) (agent.py:306-311,
rl.py:253-266): a two-agent CommunityMicrogrid whose trainers were rebuilt with other values trains each
network with its trainer's values, checked against tests/dqn_learning_ref.py driven by the same Python-random /
np.random streams in the reference's consumption order (the first 16 steps of the thesis day)."""
import random

import numpy as np
import pytest

from conftest import load_golden
from dqn_learning_ref import MixedDQNBatch
from oracle import dqn as odqn

pytestmark = pytest.mark.gpu
T = 16
VALUES = ((0.9, 0.01, 1e-4), (0.95, 0.005, 1e-5))  # (gamma, tau, learning rate) of agents 0 and 1


def _community(d):
    """test_gpu_dqn_api's construction on the day's first T steps, the trainers rebuilt with VALUES."""
    from p2pmicrogrid_amd import rl, setup
    from p2pmicrogrid_amd.agent import Agent, DQNAgent
    from p2pmicrogrid_amd.community import CommunityMicrogrid
    from p2pmicrogrid_amd.dataset import ProfileDataset
    from p2pmicrogrid_amd.environment import env
    from p2pmicrogrid_amd.heating import HeatPump, HPHeating
    from p2pmicrogrid_amd.production import PV, Prosumer
    from p2pmicrogrid_amd.rng import ReferenceRNG
    from p2pmicrogrid_amd.storage import NoStorage
    N, R = int(d["N"]), int(d["R"])
    setup.homogeneous = bool(d["homogeneous"])
    np.random.seed(42)
    random.seed(42)
    rng = ReferenceRNG()
    lr, pr = rng.community_ratings(N, setup.homogeneous)
    ds = lambda x: ProfileDataset(np.asarray(x, np.float32), np.roll(np.asarray(x, np.float32), -1, 0))  # noqa: E731
    Agent.reset_ids()
    agents = [DQNAgent(ds(d["load_w"][i][:T]), Prosumer(PV(pr[i] * 1e3, ds(d["pv_w"][i][:T]))), NoStorage(),
                       HPHeating(HeatPump(3.0, 3e3, 0.0), 21.0), max_in=max(lr[i], pr[i]) * 1.1 * 1e3,
                       max_out=-(max(lr[i], pr[i]) + 1.1e3)) for i in range(N)]
    for a, (gamma, tau, rate) in zip(agents, VALUES):
        a.trainer = rl.Trainer(a.actor, buffer_size=5 * 1000, batch_size=32, gamma=gamma, tau=tau,
                               optimizer=rl.Adam(learning_rate=rate))
    env.setup(ds(np.stack([d["env_time"][:T], d["env_tout"][:T]], axis=1)))
    return CommunityMicrogrid(list(range(T)), agents, R)


def _reference_from(com, d):
    """The reference in the engine's state (test_gpu_dqn_api._oracle_from), each network at its trainer's values."""
    eng = com._engine
    ob = MixedDQNBatch(S=1, N=eng.N, R=eng.R, load_w=d["load_w"][None, :, :T], pv_w=d["pv_w"][None, :, :T],
                       max_in=np.array([a.max_in for a in com.agents], np.float32)[None],
                       env_time=d["env_time"][None, :T], env_tout=d["env_tout"][None, :T],
                       theta0=eng.get_weights("online"))
    ob.target = eng.get_weights("target")
    ob.m, ob.v = eng.get_weights("adam_m"), eng.get_weights("adam_v")
    ob.step = eng.step
    buf, added = eng.get_buffer()
    ob.buf = buf.reshape(1, eng.N, -1, 10).copy()
    ob.added = added.reshape(1, eng.N).astype(np.int64)
    ob.t_in = np.array([[a.heating.temperature[0] for a in com.agents]], np.float32)
    ob.t_m = np.array([[a.heating.building_mass_temperature[0] for a in com.agents]], np.float32)
    ob.set_learning(gamma=[[a.trainer._gamma for a in com.agents]], tau=[[a.trainer._tau for a in com.agents]],
                    lr=[[a.trainer.optimizer.learning_rate for a in com.agents]])
    return ob


def test_community_trains_each_network_with_its_trainers_values():
    d = load_golden("loop_thesis_T96")
    N, R = int(d["N"]), int(d["R"])
    com = _community(d)
    com.init_buffers()
    eng = com._engine
    learn = eng.get_learning()
    assert [tuple(x) for x in zip(learn["gamma"][0], learn["tau"][0], learn["lr"][0])] == list(VALUES)
    assert (learn["clip"] == 1.0).all() and (learn["penalty_weight"] == 10.0).all()
    py, rs = random.Random(), np.random.RandomState()
    for episode in range(2):
        if episode == 1:  # a change between episodes is uploaded, the Adam state staying
            com.agents[1].trainer._tau = 0.25
            com.agents[0].trainer.optimizer.learning_rate = 3e-5
        ob = _reference_from(com, d)
        th0 = ob.theta.copy()
        eps = com.agents[0].actor._epsilon
        py.setstate(random.getstate())
        rs.set_state(np.random.get_state())
        codes, samples = odqn.reference_dqn_replay(py, rs, T, R, N, eps, counts=ob.count().ravel())
        reward, _ = com.train_episode()
        out = ob.run_episode("train", codes=codes[:, :, None, :], samples=samples[:, None], rng="replay")
        assert np.array_equal(com.last_rewards, out["reward"][:, 0, :])
        assert np.array_equal(com.last_losses, out["loss"][:, 0, :])
        assert reward == float(out["episode_reward"][0])
        for which, want in (("online", ob.theta), ("target", ob.target), ("adam_m", ob.m), ("adam_v", ob.v)):
            assert np.array_equal(eng.get_weights(which), want), (episode, which)
        assert not np.array_equal(ob.theta, th0) and eng.step == (episode + 1) * T
        for a in com.agents:
            a.actor.decay_exploration()
    learn = eng.get_learning()
    assert list(learn["tau"][0]) == [0.01, 0.25] and list(learn["lr"][0]) == [3e-5, 1e-5]
    assert list(learn["gamma"][0]) == [0.9, 0.95]
