"""Per-network gamma, tau, lr and clip, per-agent comfort weight and per-scenario epsilon of the DQN learner on
the device (p2pmg_dqn_set_learning, p2pmg_dqn_run_episode_eps), bit for bit against the oracle: one S = 1
OracleDQNBatch per hyper-parameter point for a sweep, tests/dqn_learning_ref.py for mixed values inside one
batch.  S = 4, N = 2, R = 1, T = 16, capacity 64: two Philox fill episodes, then two Philox train episodes.
Some agents start outside the comfort band, so the comfort weight enters the rewards from the first step."""
import ctypes as C

import numpy as np
import pytest

from dqn_learning_ref import MixedDQNBatch, per_scenario_eps
from oracle import dqn as odqn
from oracle.restatement import OracleParams
from p2pmicrogrid_amd import _lib
from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.dqn import DeviceDQNBatch
from p2pmicrogrid_amd.engine import DeviceCommunityBatch

pytestmark = pytest.mark.gpu
S, N, R, T, CAP = 4, 2, 1, 16, 64
RECORDS = ("reward", "cost", "action", "t_in", "loss")
PLAN = (("fill", 1.0), ("fill", 1.0), ("train", 0.7), ("train", 0.3))
# one hyper-parameter point per scenario; the per-scenario rates cover explore-all (1.0), never (0.0) and the
# small-epsilon action layout (0.002 < 2^-8)
GAMMA, TAU = np.array([0.95, 0.9, 0.5, 1.0]), np.array([0.005, 0.01, 0.2, 1.0])
LR, CLIP = np.array([1e-5, 1e-4, 1e-3, 3e-3]), np.array([1.0, 0.5, 1e-3, 7.0])
WEIGHT = np.array([0.0, 10.0, 2.5, 40.0], np.float32)
EPS = {"fill": np.array([1.0, 1.0, 0.9, 1.0]), "train": np.array([0.7, 0.002, 0.0, 1.0])}


def _eq(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(got, want):
        d = np.abs(got.astype(np.float64) - want)
        raise AssertionError(f"{what}: {np.count_nonzero(d)} of {d.size} differ, max |diff| {d.max():.3g}")


def _inputs(s=S, n=N, t=T):
    inp = scenario_batch(s, n, t)
    off = np.linspace(-1.6, 1.6, s * n).astype(np.float32).reshape(s, n)  # T_in from 19.4 to 22.6: both penalties
    return inp, (np.float32(21.0) + off).astype(np.float32), inp.t_m0


def _device(inp, t_in, t_m, shared=False, **kw):
    s, n = inp.max_in.shape
    eng = DeviceDQNBatch(s, n, R, inp.load_w.shape[-1], shared=shared, capacity=CAP, init_seed=5, **kw)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(t_in, t_m)
    return eng


def _oracle(cls, inp, t_in, t_m, theta0, rows=slice(None), **kw):
    s = inp.load_w[rows].shape[0]
    kw.setdefault("dqn", odqn.DQNParams(capacity=CAP))
    ob = cls(S=s, N=inp.max_in.shape[1], R=R, load_w=inp.load_w[rows], pv_w=inp.pv_w[rows], max_in=inp.max_in[rows],
             env_time=inp.time[None], env_tout=inp.t_out[rows], theta0=theta0, **kw)
    ob.t_in, ob.t_m = t_in[rows].copy(), t_m[rows].copy()
    return ob


def _state(eng):
    buf, added = eng.get_buffer()
    t_in, t_m = eng.get_temperatures()
    return {**{k: eng.get_weights(k) for k in ("online", "target", "adam_m", "adam_v")}, "buf": buf, "added": added,
            "t_in": t_in, "t_m": t_m, "steps": eng.net_steps()}


def _compare_state(st, ob, what, nets=slice(None), agents=slice(None)):
    n_ag = ob.S * ob.N
    for k, v in (("online", ob.theta), ("target", ob.target), ("adam_m", ob.m), ("adam_v", ob.v)):
        _eq(st[k][nets], v, f"{what} {k}")
    _eq(st["added"][agents], ob.added.ravel(), f"{what} added")
    held = min(int(ob.added.min()), CAP)  # the slots written so far (the device never clears the rest)
    _eq(st["buf"][agents][:, :held], ob.buf.reshape(n_ag, CAP, 10)[:, :held], f"{what} replay ring")
    _eq(st["t_in"].reshape(-1)[agents], ob.t_in.ravel(), f"{what} t_in")
    _eq(st["t_m"].reshape(-1)[agents], ob.t_m.ravel(), f"{what} t_m")


def _compare_records(rec, out, what, scen=slice(None)):
    _eq(rec["action"][:, :, scen], out["action"].astype(np.uint8), f"{what} action")
    for k in ("reward", "cost", "t_in") + (("loss",) if out["loss"].any() else ()):  # a fill episode records no loss
        _eq(rec[k][:, scen], out[k], f"{what} {k}")


def _same_records(a, b, plan, what=""):
    """Two device runs' records of every episode (a fill episode trains nothing: its loss buffer is not written)."""
    for ep, (mode, _) in enumerate(plan):
        for k in RECORDS:
            if k != "loss" or mode == "train":
                _eq(a[ep][k], b[ep][k], f"{what} episode {ep} {k}")


def _run_device(eng, plan, eps_of=None):
    """The plan's episodes on the device; returns each episode's records."""
    recs = []
    for ep, (mode, eps) in enumerate(plan):
        eng.run_episode(mode, "philox", episode=ep, epsilon=eps if eps_of is None else eps_of[mode], record=RECORDS)
        recs.append(eng.get_records(RECORDS))
    return recs


# ---------------------------------------------------------------- 1. sweep
def test_sweep_one_point_per_scenario_equals_one_oracle_run_each():
    """Scenario s trains at its own (gamma, tau, lr, clip), comfort weight and exploration rate in ONE context:
    weights, targets, Adam moments, replay rings, records and temperatures equal four S = 1 oracle runs, each
    given the scenario's global agent ids, its DQNParams, its OracleParams(penalty_weight) and its rate."""
    inp, t_in, t_m = _inputs()
    eng = _device(inp, t_in, t_m)
    theta0 = eng.get_weights("online")
    per_net = lambda x: np.repeat(np.asarray(x)[:, None], N, axis=1)  # noqa: E731
    eng.set_learning(gamma=per_net(GAMMA), tau=per_net(TAU), lr=per_net(LR), clip=per_net(CLIP), penalty_weight=per_net(WEIGHT))
    got = eng.get_learning()
    assert np.array_equal(got["gamma"], per_net(GAMMA)) and np.array_equal(got["lr"], per_net(LR))
    assert np.array_equal(got["penalty_weight"], per_net(WEIGHT)) and got["tau"].shape == (S, N)
    recs = _run_device(eng, PLAN, eps_of=EPS)
    st = _state(eng)
    eng.close()
    assert list(st["steps"]) == [2 * T] * (S * N)
    for s in range(S):
        a0, a1 = s * N, (s + 1) * N
        ob = _oracle(odqn.OracleDQNBatch, inp, t_in, t_m, theta0[a0:a1], rows=slice(s, s + 1),
                     dqn=odqn.DQNParams(gamma=GAMMA[s], tau=TAU[s], lr=LR[s], clip=CLIP[s], capacity=CAP),
                     params=OracleParams(penalty_weight=float(WEIGHT[s])))
        for ep, (mode, _) in enumerate(PLAN):
            out = ob.run_episode(mode, rng="philox", episode=ep, eps=float(EPS[mode][s]), agent_ids=np.arange(a0, a1))
            _compare_records(recs[ep], out, f"scenario {s} episode {ep}", scen=slice(s, s + 1))
        _compare_state(st, ob, f"scenario {s}", nets=slice(a0, a1), agents=slice(a0, a1))
    # the weight reached the rewards: scenarios 0 and 3 start outside the comfort band, with weights 0 and 40
    assert (recs[0]["reward"][0, 0] == -recs[0]["cost"][0, 0]).all()
    assert (recs[0]["reward"][0, 3] != -recs[0]["cost"][0, 3]).all()


# ---------------------------------------------------------------- 2, 3, 6. mixed community, schedule, greedy
MIX = dict(gamma=np.tile([0.95, 0.8], (S, 1)) - 0.01 * np.arange(S)[:, None], tau=np.tile([0.005, 0.05], (S, 1)),
           lr=np.tile([1e-5, 2e-4], (S, 1)) * (1 + np.arange(S)[:, None]), clip=np.tile([1.0, 0.01], (S, 1)),
           penalty_weight=np.tile(np.array([10.0, 1.5], np.float32), (S, 1)))
SCHEDULE = dict(lr=np.tile([5e-4, 1e-6], (S, 1)), tau=np.tile([0.5, 0.0], (S, 1)))


@pytest.fixture(scope="module")
def mixed():
    """Agents 0 and 1 of every scenario differ in all four values and in weight; after the first train episode
    set_learning(lr=, tau=) changes the schedule.  The device run and the reference run, done once."""
    inp, t_in, t_m = _inputs()
    eng = _device(inp, t_in, t_m)
    ob = _oracle(MixedDQNBatch, inp, t_in, t_m, eng.get_weights("online"))
    eng.set_learning(**MIX)
    ob.set_learning(**MIX)
    recs, outs, states = [], [], []
    for ep, (mode, eps) in enumerate(PLAN):
        if ep == 3:
            eng.set_learning(**SCHEDULE)
            ob.set_learning(**SCHEDULE)
        eng.run_episode(mode, "philox", episode=ep, epsilon=eps, record=RECORDS)
        recs.append(eng.get_records(RECORDS))
        outs.append(ob.run_episode(mode, rng="philox", episode=ep, eps=eps))
        states.append((_state(eng), {k: getattr(ob, k).copy() for k in ("theta", "target", "m", "v", "buf", "added", "t_in", "t_m")}))
    yield eng, ob, recs, outs, states, (t_in, t_m)
    eng.close()


class _Snap:
    def __init__(self, d):
        self.__dict__.update(d)
        self.S, self.N = S, N


def test_mixed_values_inside_one_community_equal_the_reference(mixed):
    _, _, recs, outs, states, _ = mixed
    for ep in range(3):  # up to and including the first train episode: the mixed rows
        _compare_records(recs[ep], outs[ep], f"episode {ep}")
        _compare_state(states[ep][0], _Snap(states[ep][1]), f"episode {ep}")
    th = states[2][0]["online"]
    assert not np.array_equal(th, states[1][0]["online"])  # it trained


def test_schedule_between_episodes_keeps_adam_state(mixed):
    """set_learning(lr=, tau=) after the first train episode: the second equals the reference run the same way,
    the Adam counts go on (2 T) and the moments continue from the first episode's."""
    eng, ob, recs, outs, states, _ = mixed
    _compare_records(recs[3], outs[3], "episode 3")
    _compare_state(states[3][0], _Snap(states[3][1]), "episode 3")
    assert list(states[3][0]["steps"]) == [2 * T] * (S * N)
    got = eng.get_learning()
    assert np.array_equal(got["lr"], SCHEDULE["lr"]) and np.array_equal(got["tau"], SCHEDULE["tau"])
    assert np.array_equal(got["gamma"], MIX["gamma"]) and np.array_equal(got["clip"], MIX["clip"])
    # tau = 0 froze agent 1's targets over the last episode, tau = 0.5 moved agent 0's
    tg2, tg3 = states[2][0]["target"].reshape(S, N, -1), states[3][0]["target"].reshape(S, N, -1)
    assert np.array_equal(tg2[:, 1], tg3[:, 1]) and not np.array_equal(tg2[:, 0], tg3[:, 0])


def test_greedy_launch_equals_stepwise_greedy_with_mixed_weights(mixed):
    """run_greedy("online") and run_episode("greedy") on the trained mixed batch, from the starting temperatures
    (scenario 0's two agents below the comfort band): the same rewards, each with its agent's own weight."""
    eng, (t_in, t_m) = mixed[0], mixed[5]
    rec = ("reward", "cost", "action", "t_in")
    eng.set_temperatures(t_in, t_m)
    eng.run_episode("greedy", record=rec)
    a = eng.get_records(rec)
    ep_a = eng.episode_reward()
    eng.set_temperatures(t_in, t_m)
    eng.run_greedy("online", record=rec)
    b = eng.get_records(rec)
    for k in rec:
        _eq(b[k], a[k], f"greedy {k}")
    _eq(eng.episode_reward(), ep_a, "episode reward")
    # step 0, scenario 0: weight * (distance below 20 degrees + 1) is about 10 * 1.6 for agent 0, 1.5 * 1.14 for agent 1
    pen = -(a["reward"].astype(np.float64) + a["cost"])[0, 0]
    assert 15.0 < pen[0] < 17.0 and 1.5 < pen[1] < 2.0, pen


# ---------------------------------------------------------------- 4. shared network
@pytest.mark.parametrize("segments", [1, 2])
def test_shared_network_row_equals_oracle(segments):
    inp, t_in, t_m = _inputs()
    dp = odqn.DQNParams(gamma=0.8, tau=0.05, lr=3e-4, clip=0.02, capacity=CAP)
    eng = _device(inp, t_in, t_m, shared=True, agents_per_block=1, grad_segments=segments)
    ob = _oracle(odqn.OracleDQNBatch, inp, t_in, t_m, eng.get_weights("online"), shared=True, agents_per_block=1,
                 grad_segments=segments, dqn=dp, params=OracleParams(penalty_weight=3.0))
    eng.set_learning(gamma=dp.gamma, tau=dp.tau, lr=dp.lr, clip=dp.clip, penalty_weight=3.0)
    assert eng.get_learning()["gamma"].shape == (1,)
    recs = _run_device(eng, PLAN)
    for ep, (mode, eps) in enumerate(PLAN):
        _compare_records(recs[ep], ob.run_episode(mode, rng="philox", episode=ep, eps=eps), f"episode {ep}")
    _compare_state(_state(eng), ob, "shared")
    eng.close()


def test_per_scenario_eps_on_the_mfma_act_kernel(monkeypatch):
    """S = 37, N = 2: the MFMA act kernel's 16 agent slots hold 8 scenarios, the last workgroup 5; every scenario
    has its own rate.  Fill, fill, train equal the one-wave-per-agent act kernel (P2PMG_DQN_ACT=wave) bit for bit;
    the two fill episodes (records, rings, temperatures: everything a rate decides) equal the oracle, whose
    shared-network training of 74 agents would take this test past ten seconds (the wave kernel's training
    with per-scenario rates is test_sweep's, against the oracle)."""
    s = 37
    inp, t_in, t_m = _inputs(s)
    eps = {"fill": np.linspace(0.5, 1.0, s), "train": np.concatenate([[0.0, 0.002, 1.0], np.linspace(0.05, 0.95, s - 3)])}
    plan = PLAN[:3]
    runs = {}
    for form in ("mfma", "wave"):
        monkeypatch.delenv("P2PMG_DQN_ACT", raising=False)
        if form == "wave":
            monkeypatch.setenv("P2PMG_DQN_ACT", "wave")
        eng = _device(inp, t_in, t_m, shared=True, agents_per_block=1)
        theta0 = eng.get_weights("online")
        recs = _run_device(eng, plan, eps_of=eps)
        assert ("dqn_act_shared_kernel" in eng.last_kernel()) == (form == "mfma"), eng.last_kernel()
        runs[form] = (recs, _state(eng))
        eng.close()
    _same_records(runs["mfma"][0], runs["wave"][0], plan, "mfma / wave")
    held = len(plan) * T  # ring slots written so far: the device never clears the rest (whatever the allocation held)
    assert list(runs["wave"][1]["added"]) == [held] * (s * N) and held < CAP
    for k, v in runs["wave"][1].items():
        if k == "buf":
            _eq(runs["mfma"][1][k][:, :held], v[:, :held], k)
        else:
            _eq(runs["mfma"][1][k], v, k)
    ob = _oracle(odqn.OracleDQNBatch, inp, t_in, t_m, theta0, shared=True, agents_per_block=1)
    with per_scenario_eps():
        for ep in range(2):
            out = ob.run_episode("fill", rng="philox", episode=ep, eps=eps["fill"][:, None])
            _compare_records(runs["mfma"][0][ep], out, f"episode {ep}")
    buf = runs["mfma"][1]["buf"]  # the train episode wrote slots 2 T .. 3 T - 1
    _eq(buf[:, :2 * T], ob.buf.reshape(s * N, CAP, 10)[:, :2 * T], "replay rings after the fill episodes")
    assert len({tuple(r.ravel()) for r in np.moveaxis(runs["mfma"][0][2]["action"], 2, 0)}) > 8  # the rates differ


# ---------------------------------------------------------------- 5. defaults
def test_defaults_untouched_and_restored_equal_the_oracle():
    inp, t_in, t_m = _inputs()
    states = []
    for form in ("never", "all-none", "restored"):
        eng = _device(inp, t_in, t_m)
        theta0 = eng.get_weights("online")
        if form == "all-none":
            eng.set_learning()
        if form == "restored":
            eng.set_learning(**MIX)
            eng.set_learning()
        recs = _run_device(eng, PLAN)
        states.append((recs, _state(eng), eng.get_learning()))
        eng.close()
    for recs, st, learn in states[1:]:
        _same_records(recs, states[0][0], PLAN)
        for k, v in states[0][1].items():
            _eq(st[k], v, k)
        for k, v in states[0][2].items():
            _eq(learn[k], v, k)
    learn = states[0][2]
    assert (learn["gamma"] == 0.95).all() and (learn["tau"] == 0.005).all() and (learn["lr"] == 1e-5).all()
    assert (learn["clip"] == 1.0).all() and (learn["penalty_weight"] == 10.0).all()
    ob = _oracle(odqn.OracleDQNBatch, inp, t_in, t_m, theta0)
    for ep, (mode, eps) in enumerate(PLAN):
        _compare_records(states[0][0][ep], ob.run_episode(mode, rng="philox", episode=ep, eps=eps), f"episode {ep}")
    _compare_state(states[0][1], ob, "defaults")


# ---------------------------------------------------------------- 7. validation
def test_validation_leaves_the_state_untouched():
    inp, t_in, t_m = _inputs()
    eng = _device(inp, t_in, t_m)
    eng.set_learning(**MIX)
    before = eng.get_learning()
    bad_w = MIX["penalty_weight"].copy()
    bad_w[2, 1] = -1.0
    nan_lr = MIX["lr"].copy()
    nan_lr[3, 0] = np.nan
    for kw, word, unit in ((dict(gamma=1.5), "gamma", "network 0"), (dict(tau=-0.1), "tau", "network 0"),
                           (dict(lr=nan_lr), "lr", "network 6"), (dict(clip=0.0), "clip", "network 0"),
                           (dict(penalty_weight=bad_w), "penalty weight", "agent 5"),
                           (dict(gamma=0.5, tau=0.5, lr=0.5, clip=0.5, penalty_weight=bad_w), "penalty weight", "agent 5")):
        with pytest.raises(_lib.P2PMGError, match="INVALID") as e:
            eng.set_learning(**kw)
        assert word in str(e.value) and unit in str(e.value), str(e.value)
        for k, v in before.items():
            _eq(eng.get_learning()[k], v, f"{k} after a rejected {sorted(kw)}")
    eps = np.full(S, 0.5)
    for mode, rng in (("greedy", "philox"), ("train", "replay"), ("fill", "replay")):
        with pytest.raises(ValueError):
            eng.run_episode(mode, rng, epsilon=eps)
    with pytest.raises(ValueError):
        eng.run_episode("fill", "philox", epsilon=eps[:-1])
    args = _lib.EpisodeArgs(_lib.MODE_GREEDY, _lib.RNG_PHILOX, 0, 0, 0.5, 0, 0)
    assert eng.L.p2pmg_dqn_run_episode_eps(eng._ctx, C.byref(args), eps) == 1                     # P2PMG_E_INVALID
    args = _lib.EpisodeArgs(_lib.MODE_TRAIN, _lib.RNG_REPLAY, 0, 0, 0.5, 0, 0)
    assert eng.L.p2pmg_dqn_run_episode_eps(eng._ctx, C.byref(args), eps) == 1
    args = _lib.EpisodeArgs(_lib.MODE_FILL, _lib.RNG_PHILOX, 0, 0, 0.5, 0, 0)
    assert eng.L.p2pmg_dqn_run_episode_eps(eng._ctx, C.byref(args), np.array([0.1, 0.2, 1.5, 0.3])) == 1
    assert b"scenario 2" in eng.L.p2pmg_last_error(eng._ctx)
    eng.close()
    tab = DeviceCommunityBatch(1, 2, 1, T)
    g = np.full(2, 0.9)
    assert tab.L.p2pmg_dqn_set_learning(tab._ctx, g.ctypes.data, None, None, None, None) == 4   # P2PMG_E_STATE
    assert tab.L.p2pmg_dqn_get_learning(tab._ctx, g.ctypes.data, None, None, None, None) == 4
    args = _lib.EpisodeArgs(_lib.MODE_TRAIN, _lib.RNG_PHILOX, 0, 0, 0.5, 0, 0)
    assert tab.L.p2pmg_dqn_run_episode_eps(tab._ctx, C.byref(args), np.full(1, 0.5)) == 4
    tab.close()
