"""One DQN network per role on the device (p2pmg_dqn_setup_roles, DeviceDQNBatch(shared="role")), bit for bit
against tests/dqn_role_ref.py::RoleDQNBatch, against the shared-network context at N = 1 and against the per-agent
context at S = 1.

A training episode is admitted only with 31 transitions per agent in memory, which one fill episode of T = 12
steps does not give, so every case that trains first loads the same seeded transitions into the device's rings
and the reference's (dqn_role_ref.preload_rings): 40 per agent where a fill episode follows (52, 64, then 76 > 64:
the second training episode evicts), 31 where none does (the first sample of 32 then takes the whole ring, the
smallest count a sample can be drawn from)."""
import ctypes as C

import numpy as np
import pytest

from dqn_learning_ref import per_scenario_eps
from dqn_role_ref import RoleDQNBatch, load_rings, preload_rings
from oracle import dqn as odqn
from oracle.restatement import OracleParams
from p2pmicrogrid_amd import _lib
from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.dqn import DeviceDQNBatch

pytestmark = pytest.mark.gpu
T, CAP, HELD = 12, 64, 40
RECORDS = ("reward", "cost", "action", "t_in", "loss")
PLAN = (("fill", 1.0), ("train", 0.7), ("train", 0.3))
STATE = ("online", "target", "adam_m", "adam_v")


def _eq(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(got, want):
        d = np.abs(got.astype(np.float64) - want) if got.shape == want.shape else np.zeros(1)
        raise AssertionError(f"{what}: shapes {got.shape} {want.shape}, {np.count_nonzero(d)} of {d.size} differ, "
                             f"max |diff| {d.max():.3g}")


def _inputs(s, n, t=T):
    inp = scenario_batch(s, n, t)
    off = np.linspace(-1.6, 1.6, s * n).astype(np.float32).reshape(s, n)  # T_in from 19.4 to 22.6: both penalties
    return inp, (np.float32(21.0) + off).astype(np.float32), inp.t_m0


def _device(inp, t_in, t_m, r, shared="role", held=HELD, **kw):
    s, n = inp.max_in.shape
    eng = DeviceDQNBatch(s, n, r, inp.load_w.shape[-1], shared=shared, capacity=CAP, init_seed=None, **kw)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(t_in, t_m)
    if held:
        eng.set_buffer(*preload_rings(s * n, CAP, held))
    return eng


def _weights(eng, theta):
    eng.set_weights("online", theta)
    eng.set_weights("target", theta)


def _oracle(inp, t_in, t_m, r, theta0, held=HELD, cls=RoleDQNBatch, **kw):
    s, n = inp.max_in.shape
    kw.setdefault("dqn", odqn.DQNParams(capacity=CAP))
    ob = cls(S=s, N=n, R=r, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in, env_time=inp.time[None],
             env_tout=inp.t_out, theta0=theta0, **kw)
    ob.t_in, ob.t_m = t_in.copy(), t_m.copy()
    if held:
        load_rings(ob, *preload_rings(s * n, CAP, held))
    return ob


def _state(eng):
    buf, added = eng.get_buffer()
    t_in, t_m = eng.get_temperatures()
    return {**{k: eng.get_weights(k) for k in STATE}, "buf": buf, "added": added, "t_in": t_in, "t_m": t_m,
            "steps": eng.net_steps()}


def _compare_state(st, ob, what):
    for k, v in (("online", ob.theta), ("target", ob.target), ("adam_m", ob.m), ("adam_v", ob.v)):
        _eq(st[k], v, f"{what} {k}")
    _eq(st["added"], ob.added.ravel(), f"{what} added")
    held = min(int(ob.added.min()), CAP)  # the slots written so far (the device never clears the rest)
    _eq(st["buf"][:, :held], ob.buf.reshape(-1, CAP, 10)[:, :held], f"{what} replay ring")
    _eq(st["t_in"], ob.t_in, f"{what} t_in")
    _eq(st["t_m"], ob.t_m, f"{what} t_m")
    _eq(st["steps"], np.full(ob.N, ob.step), f"{what} Adam step counts")


def _compare_records(rec, out, what, train):
    _eq(rec["action"], out["action"].astype(np.uint8), f"{what} action")
    for k in ("reward", "cost", "t_in") + (("loss",) if train else ()):  # a fill episode records no loss
        _eq(rec[k], out[k], f"{what} {k}")


def _same_devices(a, b, plan, what):
    (ra, sa), (rb, sb) = a, b
    for ep, (mode, _) in enumerate(plan):
        for k in RECORDS:
            if k != "loss" or mode == "train":
                _eq(ra[ep][k], rb[ep][k], f"{what} episode {ep} {k}")
    held = min(int(sa["added"].min()), CAP)
    for k in sa:
        _eq(sa[k][:, :held] if k == "buf" else sa[k], sb[k][:, :held] if k == "buf" else sb[k], f"{what} {k}")


def _run_device(eng, plan, first=0, rng="philox"):
    recs = []
    for ep, (mode, eps) in enumerate(plan):
        eng.run_episode(mode, rng, episode=first + ep, epsilon=eps, record=RECORDS)
        recs.append(eng.get_records(RECORDS))
    return recs


# ---------------------------------------------------------------- 1, 7. ragged blocks, eviction, greedy
@pytest.fixture(scope="module")
def ragged():
    """S = 5, N = 2, R = 1, T = 12, capacity 64, agents_per_block = 2: each role's blocks hold 2, 2 and 1 agents.
    One fill, two Philox training episodes and one greedy episode on the device and on the reference."""
    inp, t_in, t_m = _inputs(5, 2)
    theta0 = odqn.glorot_init(2, seed=5)
    eng = _device(inp, t_in, t_m, 1, agents_per_block=2)
    _weights(eng, theta0)
    ob = _oracle(inp, t_in, t_m, 1, theta0, agents_per_block=2)
    recs, outs = _run_device(eng, PLAN), []
    for ep, (mode, eps) in enumerate(PLAN):
        outs.append(ob.run_episode(mode, rng="philox", episode=ep, eps=eps))
    st = _state(eng)
    trained = {k: getattr(ob, k).copy() for k in ("theta", "target", "m", "v", "buf", "added", "t_in", "t_m")}
    eng.set_temperatures(t_in, t_m)
    ob.t_in, ob.t_m = t_in.copy(), t_m.copy()
    rec = ("reward", "cost", "action", "t_in")
    eng.run_episode("greedy", record=rec)
    greedy = (eng.get_records(rec), eng.episode_reward(), ob.run_episode("greedy"))
    yield eng, ob, recs, outs, st, trained, greedy, (inp, t_in, t_m)
    eng.close()


class _Snap:
    def __init__(self, d, ob):
        self.__dict__.update(d)
        self.N, self.step = ob.N, ob.step


def test_ragged_blocks_and_eviction_equal_the_reference(ragged):
    eng, ob, recs, outs, st, trained, greedy, _ = ragged
    assert eng.shared == "role" and eng.n_nets == 2
    n = C.c_int(-1)
    assert eng.L.p2pmg_dqn_roles(eng._ctx, C.byref(n)) == 0 and n.value == 2
    assert eng.grad_layout() == {"segments": 1, "agents_per_block": 2, "blocks": 2 * 3}
    assert eng.last_kernel() == "dqn_act_kernel<2,roles>"
    for ep, (mode, _) in enumerate(PLAN):
        _compare_records(recs[ep], outs[ep], f"episode {ep}", mode == "train")
    _compare_state(st, _Snap(trained, ob), "after training")
    assert int(st["added"].min()) == HELD + 3 * T > CAP  # the second training episode evicted
    assert list(st["steps"]) == [2 * T, 2 * T]
    assert not np.array_equal(st["online"][0], st["online"][1])
    assert recs[2]["loss"].all() and not np.array_equal(st["online"], odqn.glorot_init(2, seed=5))
    g_rec, g_ep, g_out = greedy
    _compare_records(g_rec, g_out, "greedy", False)
    _eq(g_ep, g_out["episode_reward"], "greedy episode reward")


def test_replayed_codes_and_samples_equal_the_reference():
    """The same shape through replay mode: uploaded exploration codes and sample indices instead of Philox."""
    inp, t_in, t_m = _inputs(5, 2)
    theta0 = odqn.glorot_init(2, seed=6)
    eng = _device(inp, t_in, t_m, 1, agents_per_block=2)
    _weights(eng, theta0)
    ob = _oracle(inp, t_in, t_m, 1, theta0, agents_per_block=2)
    rs = np.random.RandomState(11)
    codes = np.where(rs.rand(T, 2, 5, 2) < 0.5, rs.randint(0, 3, (T, 2, 5, 2)), 255).astype(np.uint8)
    # deque indices into the HELD + t + 1 transitions in memory at step t: 32 distinct ones per agent
    samples = np.stack([np.stack([rs.permutation(HELD + t + 1)[:32] for _ in range(10)]).reshape(5, 2, 32)
                        for t in range(T)])
    eng.set_replay_codes(codes)
    eng.set_samples(samples)
    eng.run_episode("train", "replay", record=RECORDS)
    out = ob.run_episode("train", codes=codes, samples=samples, rng="replay")
    _compare_records(eng.get_records(RECORDS), out, "replay", True)
    _compare_state(_state(eng), ob, "replay")
    eng.close()


# ---------------------------------------------------------------- 2. several slices, three roles, smallest samples
def test_three_roles_over_37_scenarios_from_the_smallest_memory():
    """S = 37, N = 3, R = 0, agents_per_block = 16: a role's 37 agents in blocks of 16, 16 and 5, so three of the
    reduce kernel's 16 slices hold a partial and the last block is ragged.  No fill episode: 31 transitions per
    agent are loaded, so the first training step samples all 32 in memory.  T = 4 keeps the reference's 111
    agents within seconds."""
    t = 4
    inp, t_in, t_m = _inputs(37, 3, t)
    theta0 = odqn.glorot_init(3, seed=7)
    eng = _device(inp, t_in, t_m, 0, held=31, agents_per_block=16)
    _weights(eng, theta0)
    assert eng.grad_layout() == {"segments": 1, "agents_per_block": 16, "blocks": 3 * 3}
    ob = _oracle(inp, t_in, t_m, 0, theta0, held=31, agents_per_block=16)
    eng.run_episode("train", "philox", episode=0, epsilon=0.5, record=RECORDS)
    out = ob.run_episode("train", rng="philox", episode=0, eps=0.5)
    _compare_records(eng.get_records(RECORDS), out, "S = 37", True)
    _compare_state(_state(eng), ob, "S = 37")
    assert eng.last_kernel() == "dqn_act_kernel<3,roles>"
    eng.close()


# ---------------------------------------------------------------- 3, 4. the two degenerate layouts, device to device
def test_one_role_is_the_shared_network_context(monkeypatch):
    """N = 1, S = 9, blocks of 4, 4 and 1 agents: the role context and the shared context (its act kernel
    the one-wave-per-agent form, P2PMG_DQN_ACT=wave, as a role context's always is) agree in every bit."""
    inp, t_in, t_m = _inputs(9, 1)
    theta0 = odqn.glorot_init(1, seed=8)
    runs = []
    for shared in ("role", True):
        monkeypatch.delenv("P2PMG_DQN_ACT", raising=False)
        if shared is True:
            monkeypatch.setenv("P2PMG_DQN_ACT", "wave")
        eng = _device(inp, t_in, t_m, 1, shared=shared, agents_per_block=4)
        _weights(eng, theta0)
        runs.append((_run_device(eng, PLAN), _state(eng)))
        assert eng.last_kernel() == ("dqn_act_kernel<1,roles>" if shared == "role" else "dqn_act_kernel<1>")
        layout = eng.grad_layout()
        eng.close()
        assert layout == {"segments": 1, "agents_per_block": 4, "blocks": 3}
    _same_devices(runs[0], runs[1], PLAN, "N = 1")
    assert not np.array_equal(runs[0][1]["online"], theta0)


def test_one_scenario_is_the_per_agent_context():
    """S = 1, N = 3: one agent, one block, one partial per role."""
    inp, t_in, t_m = _inputs(1, 3)
    theta0 = odqn.glorot_init(3, seed=9)
    runs = []
    for shared in ("role", False):
        eng = _device(inp, t_in, t_m, 1, shared=shared)
        _weights(eng, theta0)
        runs.append((_run_device(eng, PLAN), _state(eng)))
        eng.close()
    _same_devices(runs[0], runs[1], PLAN, "S = 1")
    assert not np.array_equal(runs[0][1]["online"], theta0)


# ---------------------------------------------------------------- 5. per-role learner constants
def test_per_role_learning_rows_and_a_change_between_episodes():
    """Every role its own gamma, tau, lr and clip (and every agent its own comfort weight); lr and tau change before
    the second training episode, the Adam state staying."""
    s, n = 3, 2
    inp, t_in, t_m = _inputs(s, n)
    theta0 = odqn.glorot_init(n, seed=10)
    mix = dict(gamma=[0.95, 0.8], tau=[0.005, 0.05], lr=[1e-5, 2e-4], clip=[1.0, 0.01],
               penalty_weight=np.array([[10.0, 1.5], [0.0, 40.0], [2.5, 10.0]], np.float32))
    change = dict(lr=[5e-4, 1e-6], tau=[0.5, 0.0])
    eng = _device(inp, t_in, t_m, 1, agents_per_block=2)
    _weights(eng, theta0)
    ob = _oracle(inp, t_in, t_m, 1, theta0, agents_per_block=2)
    got = eng.get_learning()
    assert {k: v.shape for k, v in got.items()} == {"gamma": (n,), "tau": (n,), "lr": (n,), "clip": (n,),
                                                      "penalty_weight": (s, n)}
    eng.set_learning(**mix)
    ob.set_learning(**mix)
    for ep, (mode, eps) in enumerate(PLAN):
        if ep == 2:
            eng.set_learning(**change)
            ob.set_learning(**change)
            before = eng.get_weights("target")
        eng.run_episode(mode, "philox", episode=ep, epsilon=eps, record=RECORDS)
        out = ob.run_episode(mode, rng="philox", episode=ep, eps=eps)
        _compare_records(eng.get_records(RECORDS), out, f"episode {ep}", mode == "train")
    st = _state(eng)
    _compare_state(st, ob, "per-role rows")
    got, want = eng.get_learning(), ob.get_learning()
    for k in want:
        _eq(got[k], want[k], f"get_learning {k}")
    _eq(got["lr"], change["lr"], "lr")
    _eq(got["gamma"], mix["gamma"], "gamma")
    assert np.array_equal(st["target"][1], before[1]) and not np.array_equal(st["target"][0], before[0])  # tau 0 / 0.5
    for bad in (dict(gamma=np.full(s * n, 0.9)), dict(lr=np.full((s, n), 1e-5)), dict(tau=[0.1, 0.2, 0.3]),
                dict(penalty_weight=np.zeros(n + 1, np.float32))):
        with pytest.raises(ValueError, match="broadcast"):
            eng.set_learning(**bad)
    for k, v in want.items():
        _eq(eng.get_learning()[k], v, f"{k} after refused rows")
    eng.close()


# ---------------------------------------------------------------- 6. per-scenario epsilon
def test_one_epsilon_per_scenario():
    """S = 5: explore-all, never, the small-epsilon action layout (0.002 < 2^-8) and two rates between."""
    s, n = 5, 2
    inp, t_in, t_m = _inputs(s, n)
    theta0 = odqn.glorot_init(n, seed=12)
    eps = {"fill": np.array([1.0, 0.9, 1.0, 0.5, 1.0]), "train": np.array([1.0, 0.0, 0.002, 0.3, 0.7])}
    eng = _device(inp, t_in, t_m, 1, agents_per_block=2)
    _weights(eng, theta0)
    ob = _oracle(inp, t_in, t_m, 1, theta0, agents_per_block=2)
    with per_scenario_eps():
        for ep, mode in enumerate(("fill", "train")):
            eng.run_episode(mode, "philox", episode=ep, epsilon=eps[mode], record=RECORDS)
            out = ob.run_episode(mode, rng="philox", episode=ep, eps=eps[mode][:, None])
            _compare_records(eng.get_records(RECORDS), out, f"episode {ep}", mode == "train")
    _compare_state(_state(eng), ob, "per-scenario epsilon")
    eng.close()


# ---------------------------------------------------------------- 7. greedy launch, policy set, maps
def test_greedy_launch_policy_set_and_maps(ragged):
    eng, _, _, _, st, _, greedy, (inp, t_in, t_m) = ragged
    rec = ("reward", "cost", "action", "t_in")
    g_rec, g_ep, _ = greedy  # run_episode("greedy") from the starting temperatures
    eng.set_policy_nets(eng.get_weights("online"))  # N networks: the default map is a % N
    for source in ("online", "policy"):
        eng.set_temperatures(t_in, t_m)
        eng.run_greedy(source, record=rec)
        got = eng.get_records(rec)
        for k in rec:
            _eq(got[k], g_rec[k], f'run_greedy("{source}") {k}')
        _eq(eng.episode_reward(), g_ep, f'run_greedy("{source}") episode reward')
        assert eng.last_kernel() == "dqn_greedy_episode_kernel<2>"
    eng.set_policy_nets(None)
    for k in STATE:  # nothing above wrote a network
        _eq(eng.get_weights(k), st[k], k)
    # the maps of the N networks: those of a per-agent context holding the same weights
    axes = (np.linspace(0, 1, 4), np.linspace(-1, 1, 5), np.linspace(-1, 1, 3), np.linspace(-0.5, 0.5, 3))
    eng.set_policy_grid(*axes)
    pol, q = eng.policy_map(q=True)
    stats = eng.map_stats()
    eng.map_mark()
    assert pol.shape == (2, 4, 5, 3, 3) and list(eng.map_changes(remark=False)) == [0, 0]
    per = DeviceDQNBatch(1, 2, 1, T, capacity=CAP, init_seed=None)
    per.set_weights("online", st["online"])
    per.set_policy_grid(*axes)
    pol2, q2 = per.policy_map(q=True)
    stats2 = per.map_stats()
    per.close()
    _eq(pol, pol2, "policy map")
    _eq(q, q2, "map Q values")
    for k in stats:
        _eq(stats[k], stats2[k], f"map stats {k}")
    _eq(eng.policy_map(first=1, count=1, which="target")[0].shape, pol[1].shape, "target map shape")
    # one network's forward and single-batch training address [0, N)
    x = np.random.RandomState(0).uniform(-1, 1, (7, 5)).astype(np.float32)
    _eq(eng.forward(x, net=1), odqn.api_forward(st["online"][1], x), "forward on network 1")


# ---------------------------------------------------------------- 8. refusals
def test_refusals():
    L = _lib.lib()
    inp, t_in, t_m = _inputs(2, 2)
    with pytest.raises(_lib.P2PMGError, match="INVALID.*grad_segments"):
        DeviceDQNBatch(2, 2, 1, T, shared="role", capacity=CAP, grad_segments=2)
    eng = _device(inp, t_in, t_m, 1, held=0)
    dc = _lib.DqnConfig()
    L.p2pmg_dqn_config_default(C.byref(dc))
    assert L.p2pmg_dqn_setup_roles(eng._ctx, C.byref(dc)) == 4                       # P2PMG_E_STATE: set up already
    assert b"already set up" in L.p2pmg_last_error(eng._ctx)
    # network index N, ranges past N
    w = np.zeros((3, _lib.DQN_PARAMS), np.float32)
    assert L.p2pmg_dqn_set_weights(eng._ctx, _lib.DQN_ONLINE, 0, 3, w.ctypes.data) == 1
    assert L.p2pmg_dqn_get_weights(eng._ctx, _lib.DQN_ONLINE, 2, 1, w.ctypes.data) == 1
    steps = np.zeros(3, np.int64)
    assert L.p2pmg_dqn_get_net_steps(eng._ctx, 1, 2, steps.ctypes.data) == 1
    x, q = np.zeros((1, 5), np.float32), np.zeros(1, np.float32)
    assert L.p2pmg_dqn_forward(eng._ctx, 2, 1, x.ctypes.data, q.ctypes.data) == 1
    batch, loss = np.zeros((32, 10), np.float32), C.c_float(0)
    assert L.p2pmg_dqn_train_batch(eng._ctx, 2, batch.ctypes.data, C.byref(loss)) == 1
    with pytest.raises(ValueError):
        eng.policy_map(first=1, count=2)
    pol = np.zeros(1 << 20, np.uint8)
    assert L.p2pmg_dqn_policy_map(eng._ctx, _lib.DQN_ONLINE, 2, 1, pol.ctypes.data, None) == 1
    # one rank only: a communicator, or an exchange over two ranks
    uid = (C.c_uint8 * 128)()
    assert L.p2pmg_comm_init(eng._ctx, uid, 0, 1) == 5                               # P2PMG_E_UNSUPPORTED
    assert b"one rank" in L.p2pmg_last_error(eng._ctx)
    with pytest.raises(_lib.P2PMGError, match="UNSUPPORTED"):
        eng.set_grad_exchange(lambda segs: None, 0, 2)
    eng.set_grad_exchange(lambda segs: None, 0, 1)  # one rank of one: accepted, never called
    eng.set_grad_exchange(None, 0, 1)
    with pytest.raises(_lib.P2PMGError, match="STATE"):  # empty rings: the existing rule for a training episode
        eng.run_episode("train", "philox")
    eng.close()
    per = DeviceDQNBatch(2, 2, 1, T, capacity=CAP)  # shared_q = 0: a network per agent
    assert L.p2pmg_dqn_setup_roles(per._ctx, C.byref(dc)) == 4                       # set up: the state comes first
    n = C.c_int(-1)
    assert L.p2pmg_dqn_roles(per._ctx, C.byref(n)) == 0 and n.value == 0
    per.close()
    # a context created with shared_q = 0 and not set up: P2PMG_E_INVALID; a tabular one: P2PMG_E_STATE
    from p2pmicrogrid_amd.engine import DeviceCommunityBatch
    raw = DeviceCommunityBatch(2, 2, 1, T, q_dtype="f32", learner=_lib.LEARNER_DQN)
    assert L.p2pmg_dqn_setup_roles(raw._ctx, C.byref(dc)) == 1 and b"shared_q" in L.p2pmg_last_error(raw._ctx)
    raw.close()
    tab = DeviceCommunityBatch(2, 2, 1, T)
    assert L.p2pmg_dqn_setup_roles(tab._ctx, C.byref(dc)) == 4
    assert L.p2pmg_dqn_roles(tab._ctx, C.byref(n)) == 0 and n.value == 0
    tab.close()
    # p2pmg_create with P2PMG_SHARED_ROLE and the DQN learner: status 5, as before
    with pytest.raises(_lib.P2PMGError, match="UNSUPPORTED"):
        DeviceCommunityBatch(2, 2, 1, T, q_dtype="f32", shared_q="role", learner=_lib.LEARNER_DQN)
    cfg = _lib.Config()
    L.p2pmg_config_default(C.byref(cfg))
    cfg.shared_q, cfg.learner = _lib.SHARED_ROLE, _lib.LEARNER_DQN
    ctx = C.c_void_p()
    assert L.p2pmg_create(C.byref(cfg), 0, C.byref(ctx)) == 5 and not ctx.value
