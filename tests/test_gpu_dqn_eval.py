"""DQN evaluation in one launch (p2pmg_dqn_run_greedy, dqn_greedy_episode_kernel) against the stepwise greedy
episode (p2pmg_run_episode, T act launches): records, final temperatures and episode rewards bit for bit, on
the context's own networks and on a policy set; the learner's state untouched; the errors.

Every case's reference side shows all three actions (dqn_eval_cases.actions_needed: the N = 1, T = 1 case
has two decisions and is held to two), so a constant policy cannot hide a wrong network or W2 column."""
import numpy as np
import pytest

import dqn_eval_cases as dc
from p2pmicrogrid_amd import _lib
from p2pmicrogrid_amd.dqn import DeviceDQNBatch
from p2pmicrogrid_amd.engine import DeviceCommunityBatch

pytestmark = pytest.mark.gpu
F32 = np.float32
REC = dc.RECORDS


def _engine(c, theta, shared=None, **kw):
    shared = c.shared if shared is None else shared
    # capacity 32: the learner test's 48 transitions per agent write every ring slot (a ring is not cleared
    # when it is allocated, so an unwritten slot would hold whatever the allocation held)
    eng = DeviceDQNBatch(c.S, c.N, c.R, c.T, shared=shared, capacity=32, init_seed=None, **kw)
    eng.set_weights("online", theta)
    eng.set_weights("target", theta)
    dc.load(eng, c)
    return eng


def _state(eng):
    """Everything an episode leaves behind that the tests compare."""
    out = dict(eng.get_records(REC))
    out["t_in_final"], out["t_m_final"] = eng.get_temperatures()
    out["episode_reward"] = eng.episode_reward()
    return out


def _same(got, want, tag=""):
    assert got.keys() == want.keys()
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, k)
        assert a.tobytes() == b.tobytes(), (tag, k, int(np.count_nonzero(a != b)), "values differ")


def _shows_actions(c, action):
    seen = np.unique(action)
    assert len(seen) >= dc.actions_needed(c), (c, seen)


def _stepwise(c, theta, episodes=1):
    eng = _engine(c, theta)
    for _ in range(episodes):
        eng.run_episode("greedy", record=REC)
    want = _state(eng)
    eng.close()
    _shows_actions(c, want["action"])
    return want


@pytest.mark.parametrize("name", list(dc.CASES))
def test_run_greedy_online_equals_the_stepwise_episode(name):
    c = dc.CASES[name]
    theta = dc.case_weights(c)
    want = _stepwise(c, theta)
    eng = _engine(c, theta)
    eng.run_greedy("online", record=REC)
    assert eng.last_kernel() == f"dqn_greedy_episode_kernel<{c.N}>"
    _same(_state(eng), want, name)
    eng.close()


def test_policy_set_with_the_role_map():
    """M = N networks, agent i of every scenario on network i: the per-agent context with the weights tiled,
    and the oracle's greedy episode on the same tiled weights (default thermal values)."""
    c = dc.ROLE
    nets = dc.weights(c.N, c.seed, c.scale)
    want = _stepwise(c, dc.tiled(nets, c.S))
    eng = _engine(c, dc.weights(c.S * c.N, 99, 1.0))  # its own networks are others: the set must be read
    eng.set_policy_nets(nets)
    w, m = eng.policy_nets()
    assert np.array_equal(w, nets) and np.array_equal(m, np.arange(c.S * c.N) % c.N) and m.dtype == np.int32
    eng.run_greedy("policy", record=REC)
    got = _state(eng)
    _same(got, want, "role map")
    out = dc.oracle_batch(c, dc.tiled(nets, c.S)).run_episode("greedy")
    assert np.array_equal(got["action"], out["action"].astype(np.uint8))
    for k in ("reward", "cost", "grid", "p2p", "t_in", "episode_reward"):
        assert got[k].tobytes() == np.asarray(out[k], F32).tobytes(), k
    eng.close()


def test_policy_set_with_an_arbitrary_map():
    c = dc.ARBITRARY
    nets = dc.weights(2, c.seed, c.scale)
    want = _stepwise(c, nets[dc.ARBITRARY_MAP])
    eng = _engine(c, dc.weights(c.S * c.N, 98, 1.0))
    eng.set_policy_nets(nets, dc.ARBITRARY_MAP)
    eng.run_greedy("policy", record=REC)
    _same(_state(eng), want, "arbitrary map")
    eng.close()


def test_source_target_reads_the_target_network():
    c = dc.CASES["s3n2r1t12"]
    online, target = dc.case_weights(c), dc.weights(c.S * c.N, c.seed + 50, c.scale)
    want = _stepwise(c, target)
    eng = _engine(c, online)
    eng.set_weights("target", target)
    eng.run_greedy("target", record=REC)
    got = _state(eng)
    _same(got, want, "target")
    eng.close()
    assert got["action"].tobytes() != _stepwise(c, online)["action"].tobytes()  # the two networks do differ


def test_two_run_greedy_calls_carry_the_state_over():
    c = dc.CASES["s2n3r0t5_odd_T"]
    theta = dc.case_weights(c)
    want = _stepwise(c, theta, episodes=2)
    eng = _engine(c, theta)
    eng.run_greedy("online", record=REC)
    eng.run_greedy("online", record=REC)
    _same(_state(eng), want, "second episode")
    eng.close()


def _learner(eng):
    buf, added = eng.get_buffer()
    return {**{w: eng.get_weights(w) for w in ("online", "target", "adam_m", "adam_v")}, "steps": eng.net_steps(),
            "buf": buf, "added": added}


def test_the_learner_is_untouched():
    """Weights, Adam state and counts, replay rings and `added` are bit-identical across run_greedy, and a
    Philox training episode after it equals the same episode on a twin context that never evaluated."""
    c = dc.CASES["s3n2r1t12"]
    theta = dc.case_weights(c)
    inp = dc.inputs(c)
    engs = []
    for _ in range(2):
        eng = _engine(c, theta, lr=1e-3)
        eng.set_weights("target", dc.weights(c.S * c.N, 77, c.scale))
        for ep in range(3):  # 36 transitions per agent: enough to sample 32
            eng.run_episode("fill", "philox", episode=ep, epsilon=1.0)
        eng.run_episode("train", "philox", episode=3, epsilon=0.5)  # Adam moments and step counts away from 0
        engs.append(eng)
    eng, twin = engs
    before = _learner(eng)
    eng.set_policy_nets(dc.weights(c.N, 5, c.scale))
    for source in ("online", "target", "policy"):
        eng.run_greedy(source, record=REC)
    _same(_learner(eng), before, "learner state")
    _same(_learner(twin), before, "twin")
    for e in (eng, twin):  # greedy evaluation moves the temperatures: both start the episode from the same
        e.set_temperatures(inp.t_in0, inp.t_m0)
        e.run_episode("train", "philox", episode=4, epsilon=0.3, record=REC + ("loss",))
    _same({**_learner(eng), **eng.get_records(REC + ("loss",))}, {**_learner(twin), **twin.get_records(REC + ("loss",))},
          "training after evaluation")
    assert not np.array_equal(_learner(eng)["online"], before["online"])
    eng.close()
    twin.close()


def test_summary_and_day_profile_after_run_greedy():
    c = dc.CASES["s3n2r1t12"]
    theta = dc.case_weights(c)
    ref = _engine(c, theta)
    ref.run_episode("greedy", record=REC)
    eng = _engine(c, theta)
    eng.run_greedy("online", record=REC)
    assert eng.last_kernel().startswith("dqn_greedy_episode_kernel<")
    assert eng.last_kernel_ms() > 0.0
    s_got, s_want = eng.episode_summary(), ref.episode_summary()
    for part in ("agent", "scenario"):
        _same(s_got[part], s_want[part], part)
    for period in (None, 4):
        for a, b in zip(eng.day_profile(period=period), ref.day_profile(period=period)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), period
    eng.close()
    ref.close()


def test_errors():
    c = dc.CASES["s3n2r1t12"]
    theta = dc.case_weights(c)
    eng = _engine(c, theta)
    L, ctx = eng.L, eng._ctx
    assert eng.policy_nets() is None
    assert L.p2pmg_dqn_run_greedy(ctx, _lib.DQN_POLICY_SET, 0) == 4  # P2PMG_E_STATE: no set yet
    with pytest.raises(_lib.P2PMGError, match="STATE"):
        eng.run_greedy("policy")
    nets = dc.weights(2, 1, 1.0)
    eng.set_policy_nets(nets, [0, 1, 1, 0, 1, 0])
    bad = [0, 1, 1, 0, 1, 2]  # a value equal to count
    with pytest.raises(_lib.P2PMGError, match="INVALID"):
        eng.set_policy_nets(dc.weights(2, 2, 1.0), bad)
    with pytest.raises(_lib.P2PMGError, match="INVALID"):
        eng.set_policy_nets(dc.weights(2, 2, 1.0), [0, -1, 1, 0, 1, 0])
    w, m = eng.policy_nets()
    assert np.array_equal(w, nets) and list(m) == [0, 1, 1, 0, 1, 0]  # the set is unchanged
    with pytest.raises(ValueError):  # 4 networks for N = 2, A = 6: no default map
        eng.set_policy_nets(dc.weights(4, 2, 1.0))
    with pytest.raises(_lib.P2PMGError, match="INVALID"):
        eng.run_greedy("online", record=("loss",))
    assert L.p2pmg_dqn_run_greedy(ctx, 7, 0) == 1 and L.p2pmg_dqn_run_greedy(ctx, _lib.DQN_ADAM_M, 0) == 1
    with pytest.raises(ValueError):
        eng.run_greedy("adam_m")
    eng.set_policy_nets(None)  # count == 0 drops the set
    assert eng.policy_nets() is None and L.p2pmg_dqn_run_greedy(ctx, _lib.DQN_POLICY_SET, 0) == 4
    eng.close()
    tab = DeviceCommunityBatch(1, 2, 0, 4, q_dtype="f32")
    n = np.zeros(1, np.int32)
    assert L.p2pmg_dqn_run_greedy(tab._ctx, _lib.DQN_ONLINE, 0) == 4
    assert L.p2pmg_dqn_set_policy_nets(tab._ctx, 1, nets.ctypes.data, None) == 4
    assert L.p2pmg_dqn_get_policy_nets(tab._ctx, n.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int)), None, None) == 4
    tab.close()
