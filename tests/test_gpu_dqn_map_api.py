"""The policy map through the object API: ActorModel.policy_map / map_stats bound and unbound,
CommunityMicrogrid.policy_maps on a DQN community, and a tabular community's refusal."""
import numpy as np
import pytest

import dqn_map_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
SMALL = (np.array([0.1, 0.6], F32), np.array([-1.2, 0.0, 0.7], F32), np.array([-0.5, 0.5], F32),
         np.array([-0.3, 0.0, 0.3, 1.1], F32))


def test_actor_model_policy_map_unbound_and_bound():
    from p2pmicrogrid_amd import rl
    from p2pmicrogrid_amd.dqn import DeviceDQNBatch
    actor = rl.ActorModel(0.1)
    th = actor.q_network.flat_weights()
    wpol, wq, wst = ref.map_ref(th, SMALL)
    pol, q = actor.policy_map(grid=SMALL, q=True)                # unbound: a one-network engine of its own
    assert pol.shape == (2, 3, 2, 4) and np.array_equal(pol, wpol) and ref.same_bits(q, wq)
    st = actor.map_stats(grid=SMALL)
    for k in ref.STAT_KEYS:
        assert np.array_equal(np.asarray(st[k]), np.asarray(wst[k])), k
    assert actor.policy_map().shape == (20, 20, 20, 20)          # the default grid: QActor.greedy_policy's shape

    eng = DeviceDQNBatch(1, 2, 0, 1, init_seed=3)
    actor.q_network.bind(eng, "online", 1)
    eng.set_policy_grid(*SMALL)
    assert np.array_equal(actor.policy_map(), wpol)              # bound: slot 1 of the engine, on its grid
    assert np.array_equal(eng.policy_map(first=1, count=1)[0], wpol)
    other = tuple(a[::-1].copy() for a in SMALL)
    assert np.array_equal(actor.policy_map(grid=other), wpol[::-1, ::-1, ::-1, ::-1])
    assert all(np.array_equal(a, b) for a, b in zip(eng.policy_grid(), SMALL))  # the engine kept its grid
    eng.close()


def _community(agent_cls, n=2):
    """A two-agent community on the thesis fixture's profiles (the construction of test_gpu_dqn_api)."""
    import random

    from conftest import load_golden
    from p2pmicrogrid_amd import setup
    from p2pmicrogrid_amd.agent import Agent
    from p2pmicrogrid_amd.community import CommunityMicrogrid
    from p2pmicrogrid_amd.dataset import ProfileDataset
    from p2pmicrogrid_amd.environment import env
    from p2pmicrogrid_amd.heating import HeatPump, HPHeating
    from p2pmicrogrid_amd.production import PV, Prosumer
    from p2pmicrogrid_amd.rng import ReferenceRNG
    from p2pmicrogrid_amd.storage import NoStorage
    d = load_golden("loop_thesis_T96")
    R, T = int(d["R"]), int(d["T"])
    setup.homogeneous = bool(d["homogeneous"])
    np.random.seed(42)
    random.seed(42)
    rng = ReferenceRNG()
    lr, pr = rng.community_ratings(n, setup.homogeneous)
    ds = lambda x: ProfileDataset(np.asarray(x, F32), np.roll(np.asarray(x, F32), -1, 0))  # noqa: E731
    Agent.reset_ids()
    agents = [agent_cls(ds(d["load_w"][i]), Prosumer(PV(pr[i] * 1e3, ds(d["pv_w"][i]))), NoStorage(),
                        HPHeating(HeatPump(3.0, 3e3, 0.0), 21.0), max_in=max(lr[i], pr[i]) * 1.1 * 1e3,
                        max_out=-(max(lr[i], pr[i]) + 1.1e3)) for i in range(n)]
    env.setup(ds(np.stack([d["env_time"], d["env_tout"]], axis=1)))
    return CommunityMicrogrid(list(range(T)), agents, R)


def test_community_policy_maps():
    from p2pmicrogrid_amd.agent import DQNAgent, QAgent
    com = _community(DQNAgent)
    want = [ref.map_ref(a.actor.q_network.flat_weights(), SMALL) for a in com.agents]
    pol, q = com.policy_maps(grid=SMALL, q=True)
    assert pol.shape == (2, 2, 3, 2, 4) and q.shape == (2, 2, 3, 2, 4, 3)
    for k in range(2):
        assert np.array_equal(pol[k], want[k][0]) and ref.same_bits(q[k], want[k][1]), k
    eng = com._ensure_engine()                                   # the networks move to the community's engine
    eng.set_policy_grid(*SMALL)
    assert np.array_equal(com.policy_maps(), pol)
    assert not np.array_equal(pol[0], pol[1]) or not ref.same_bits(q[0], q[1])
    tab = _community(QAgent)
    with pytest.raises(RuntimeError, match="DQN"):
        tab.policy_maps()
