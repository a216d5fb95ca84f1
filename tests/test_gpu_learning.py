"""Per-agent alpha, gamma and comfort weight (p2pmg_set_learning) and per-scenario epsilon
(p2pmg_run_episodes_eps) on the device against the oracle, bit for bit.

The oracle takes the learner constants as [S, N] arrays in OracleParams(alpha=..., gamma=...,
penalty_weight=...).  Philox mode draws with one epsilon per oracle run (oracle/philox.py::launch_eps),
so a batch with mixed epsilons is checked against one one-scenario OracleBatch per scenario, whose
Philox counters carry the scenario's global agent ids.  The values differ between the agents of a
community, and the initial temperatures are setpoint + 0.8 randn, so the comfort penalty is active
from step 0 and a kernel that ignored the per-agent array could not pass."""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import philox
from oracle.restatement import OracleBatch, OracleParams
from p2pmicrogrid_amd import _lib
from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.dqn import DeviceDQNBatch
from p2pmicrogrid_amd.engine import DeviceCommunityBatch, unpack_index

pytestmark = pytest.mark.gpu
F32 = np.float32
REC = ["reward", "cost", "grid", "p2p", "t_in", "action", "index"]
ALPHAS = (1e-5, 1e-3, 0.05, 0.5)
GAMMAS = (0.0, 0.5, 0.9, 0.99)
PENALTIES = (0.0, 1.0, 10.0, 100.0)
S, T = 12, 24
TRAIN_EPS = (0.81, 0.5, 0.1)


def _draw(S, N, seed=77):
    """alpha, gamma [S, N] f64, penalty [S, N] f32, T0 [S, N] f32; the agents of a community differ."""
    rs = np.random.RandomState(seed)
    alpha, gamma = rs.choice(ALPHAS, (S, N)), rs.choice(GAMMAS, (S, N))
    pen = rs.choice(PENALTIES, (S, N)).astype(F32)
    if N > 1:
        alpha[:, 0], alpha[:, -1] = 1e-5, 0.5
        gamma[:, 0], gamma[:, -1] = 0.9, 0.5
        pen[:, 0], pen[:, -1] = 10.0, 100.0
    t0 = (21.0 + 0.8 * rs.randn(S, N)).astype(F32)
    return alpha, gamma, pen, t0


def _oracle(inp, N, R, q_dtype, lr, rows=slice(None), **kw):
    alpha, gamma, pen, _ = lr
    n = inp.load_w[rows].shape[0]
    par = OracleParams(alpha=alpha[rows], gamma=gamma[rows], penalty_weight=pen[rows])
    return OracleBatch(S=n, N=N, R=R, load_w=inp.load_w[rows], pv_w=inp.pv_w[rows], max_in=inp.max_in[rows],
                       env_time=inp.time[None], env_tout=inp.t_out[rows], q_dtype=q_dtype, params=par, **kw)


def _device(inp, N, R, q_dtype="f64", lr=None, battery=None, **kw):
    S, T = inp.load_w.shape[0], inp.load_w.shape[-1]
    eng = DeviceCommunityBatch(S, N, R, T, q_dtype=q_dtype, **kw)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    if battery is not None:
        eng.set_battery(battery, 0.1, 0.9, 0.9)
    if lr is not None:
        eng.set_learning(lr[0], lr[1], lr[2])
        eng.set_temperatures(lr[3], lr[3])
    return eng


def _compare(out, rec, tag):
    for k in ("reward", "cost", "grid", "p2p", "t_in"):
        assert np.array_equal(rec[k], out[k]), (tag, k)
    assert np.array_equal(rec["action"], out["action"].astype(np.uint8)), tag
    assert np.array_equal(unpack_index(rec["index"]), out["idx"]), tag


# ----------------------------------------------------------------- 1. the arrays against the oracle
@functools.lru_cache(maxsize=None)
def _array_reference(N, R, q_dtype, battery, shared):
    """Three Philox training episodes and a greedy one in the oracle, computed once per shape and
    shared by the kernel forms and Philox placements.  Nothing downstream modifies it."""
    inp = scenario_batch(S, N, T, seed=7)
    lr = _draw(S, N)
    cap = np.full((S, N), 10 * 3.6e6) if battery else None
    ob = _oracle(inp, N, R, q_dtype, lr, shared_q=shared, battery_capacity=cap)
    ob.t_in, ob.t_m = lr[3].copy(), lr[3].copy()
    plain = OracleBatch(S=S, N=N, R=R, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in, env_time=inp.time[None],
                        env_tout=inp.t_out, q_dtype=q_dtype, shared_q=shared, battery_capacity=cap)
    plain.t_in, plain.t_m = lr[3].copy(), lr[3].copy()
    outs, deltas = [], []
    for e, eps in enumerate(TRAIN_EPS):
        outs.append(ob.run_episode("train", rng="philox", seed=42, episode=e, eps=eps))
        if shared:
            deltas.append(ob.q_delta.copy())
            ob.apply_q_delta()
    dflt = plain.run_episode("train", rng="philox", seed=42, episode=0, eps=TRAIN_EPS[0])
    assert not np.array_equal(outs[0]["reward"], dflt["reward"])  # the comfort weights matter on these inputs
    if not shared:
        assert not np.array_equal(ob.q, plain.q)
    greedy = ob.run_episode("greedy")
    return inp, lr, cap, outs, deltas, greedy, ob.q.copy()


# (N, R, q_dtype, battery, shared_q, kernel): the fast family plain (N = 2), with an idle lane (N = 3,
# R = 0), with a battery (N = 4) and at N = 5, R = 2; the general kernel's register form at N = 2 and 16,
# its tile form at N = 9, and its shared-table form at N = 16, where the arrays take sq16's place
ARRAY_CASES = [
    (2, 1, "f64", False, False, "auto"), (2, 1, "f32", False, False, "auto"),
    (3, 0, "f64", False, False, "auto"), (3, 0, "f32", False, False, "auto"),
    (4, 1, "f64", True, False, "auto"),
    (5, 2, "f64", False, False, "auto"),
    (2, 1, "f64", False, False, "general"),
    (16, 1, "f32", False, False, "auto"),
    (9, 1, "f32", False, False, "auto"),
    (16, 1, "f32", False, True, "auto"),
]


@pytest.mark.parametrize("N,R,q_dtype,battery,shared,kernel", ARRAY_CASES)
def test_learning_arrays_match_oracle(N, R, q_dtype, battery, shared, kernel):
    inp, lr, cap, outs, deltas, greedy, q_final = _array_reference(N, R, q_dtype, battery, shared)
    for placement in ("prepass", "inkernel"):
        tag = (N, R, q_dtype, battery, shared, kernel, placement)
        eng = _device(inp, N, R, q_dtype, lr=lr, battery=cap, shared_q=shared)
        got = eng.get_learning()
        assert np.array_equal(got["alpha"], lr[0]) and np.array_equal(got["gamma"], lr[1])
        assert np.array_equal(got["penalty_weight"], lr[2])
        for e, eps in enumerate(TRAIN_EPS):
            eng.run_episode("train", "philox", episode=e, epsilon=eps, record=REC, philox=placement, kernel=kernel)
            name = eng.last_kernel()
            if shared:
                assert name.startswith("episode_kernel<"), name
            elif kernel == "auto" and N <= 8 and placement == "prepass":
                assert name.startswith("episode_fast_kernel<"), name
            elif N == 9:
                assert name.startswith("episode_kernel<9,tile16"), name
            _compare(outs[e], eng.get_records(REC), tag + (e,))
            assert np.array_equal(eng.episode_reward(), outs[e]["episode_reward"]), tag
            a, b = eng.get_temperatures()
            assert np.array_equal(a, outs[e]["t_in_final"]) and np.array_equal(b, outs[e]["t_m_final"]), tag
            if shared:
                assert np.array_equal(eng.get_q_delta().reshape(-1, 3), deltas[e]), tag
                eng.apply_q_delta()
        q = eng.get_q(dtype=np.float64 if q_dtype == "f64" else np.float32)
        assert np.array_equal(q.reshape(q_final.shape), q_final), tag
        eng.run_episode("greedy", record=REC, kernel=kernel)
        _compare(greedy, eng.get_records(REC), tag + ("greedy",))
        eng.close()


def test_role_tables_sum_each_agents_own_update():
    """shared_q="role" at N = 3: the oracle has no per-role form, so role i's int64 delta is rebuilt in
    NumPy from the launch's own records with agent (s, i)'s alpha and gamma (include/p2pmg.h:
    llrint(alpha ((r + gamma max Q_i[ns]) - Q_i[s, a]) 2^40)); the rewards carry the comfort weights."""
    N, R = 3, 1
    inp = scenario_batch(S, N, T, seed=7)
    lr = _draw(S, N)
    alpha, gamma, pen, t0 = lr
    rs = np.random.RandomState(3)
    tables = rs.uniform(-1.0, 1.0, (N, 20, 20, 20, 20, 3))
    eng = _device(inp, N, R, lr=lr, shared_q="role")
    eng.set_q(tables)
    eng.run_episode("train", "philox", episode=0, epsilon=0.5, record=REC)
    assert eng.last_kernel().startswith("episode_kernel<") and ",roles" in eng.last_kernel()
    rec = eng.get_records(REC)
    # the reward is the oracle's with the agent's own weight (agent.py:225-232)
    pen_deg = np.maximum(np.maximum(F32(0), F32(20) - rec["t_in"]), np.maximum(F32(0), rec["t_in"] - F32(22)))
    pen_t = np.where(pen_deg > 0, pen_deg + F32(1), F32(0)).astype(F32)
    assert np.array_equal(rec["reward"], -(rec["cost"] + pen[None] * pen_t))
    idx = unpack_index(rec["index"])  # [T, R+1, S, N, 4]
    q = tables.reshape(N, -1, 3)
    want = np.zeros((N, 20 ** 4, 3), np.int64)
    row = lambda it, iT, ib, ip: ((it * 20 + iT) * 20 + ib) * 20 + ip
    ip0 = idx[0, 0, ..., 3]  # round 0 sees no proposals: the next state's p2p bin
    for t in range(T):
        cur, nxt = idx[t, R], idx[(t + 1) % T, 0]
        srow = row(cur[..., 0], cur[..., 1], cur[..., 2], cur[..., 3])
        nrow = row(nxt[..., 0], cur[..., 1], nxt[..., 2], ip0)
        act = rec["action"][t, R].astype(np.int64)
        for i in range(N):
            qsa = q[i][srow[:, i], act[:, i]]
            d = alpha[:, i] * ((rec["reward"][t, :, i].astype(np.float64) + gamma[:, i] * q[i][nrow[:, i]].max(-1)) - qsa)
            np.add.at(want[i], (srow[:, i], act[:, i]), np.rint(d * 2.0 ** 40).astype(np.int64))
    assert np.array_equal(eng.get_q_delta().reshape(N, -1, 3), want)
    eng.close()


# ----------------------------------------------------------------- 2. per-scenario epsilon
EPS_VALUES = (0.0, 2.0 ** -10, 0.1, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def _eps_reference(N, R, q_dtype, reset):
    """n = 3 episodes, epsilon drawn per scenario and episode: one one-scenario oracle per scenario."""
    n = 3
    inp = scenario_batch(S, N, T, seed=9)
    lr = _draw(S, N, seed=78)
    rs = np.random.RandomState(5)
    eps = rs.choice(EPS_VALUES, (n, S))
    eps[:, 0], eps[:, 1] = (1.0, 0.0, 2.0 ** -10), (2.0 ** -10, 1.0, 0.5)  # every value in every episode's mix
    rewards = np.zeros((n, S), F32)
    q, t_in, t_m, last = [], [], [], []
    for s in range(S):
        ob = _oracle(inp, N, R, q_dtype, lr, rows=slice(s, s + 1))
        ob.t_in, ob.t_m = lr[3][s:s + 1].copy(), lr[3][s:s + 1].copy()
        ids = s * N + np.arange(N)
        for k in range(n):
            out = ob.run_episode("train", rng="philox", seed=42, episode=k, eps=float(eps[k, s]), agent_ids=ids)
            rewards[k, s] = out["episode_reward"][0]
            if reset:
                a, b = philox.t0_draws(42, k + 1, ids, setpoint=21.0, sigma=0.3)
                ob.t_in, ob.t_m = a.reshape(1, N).astype(F32), b.reshape(1, N).astype(F32)
        q.append(ob.q.copy())
        t_in.append(ob.t_in[0])
        t_m.append(ob.t_m[0])
        last.append(out)
    return inp, lr, eps, rewards, np.concatenate(q), np.stack(t_in), np.stack(t_m), last


@pytest.mark.parametrize("N,R,q_dtype,reset,kernel,placement", [
    (2, 1, "f64", True, "auto", "auto"),
    (2, 1, "f64", True, "general", "prepass"), (2, 1, "f64", True, "general", "inkernel"),
    (9, 1, "f32", False, "auto", "prepass"), (9, 1, "f32", False, "auto", "inkernel"),
])
def test_per_scenario_epsilon_matches_oracle(N, R, q_dtype, reset, kernel, placement):
    inp, lr, eps, rewards, q, t_in, t_m, last = _eps_reference(N, R, q_dtype, reset)
    eng = _device(inp, N, R, q_dtype, lr=lr)
    eng.run_episodes(0, eps, reset_sigma=0.3 if reset else None, record=REC, philox=placement, kernel=kernel)
    name = eng.last_kernel()
    assert name.startswith("episode_fast_kernel<" if kernel == "auto" and N <= 8 else "episode_kernel<"), name
    assert np.array_equal(eng.episode_rewards(), rewards)
    assert np.array_equal(eng.episode_reward(), rewards[-1])
    got = eng.get_q(dtype=np.float64 if q_dtype == "f64" else np.float32)
    assert np.array_equal(got.reshape(q.shape), q)
    a, b = eng.get_temperatures()
    assert np.array_equal(a, t_in) and np.array_equal(b, t_m)
    rec = eng.get_records(REC)
    for s in range(S):  # the last episode's records, scenario by scenario
        _compare(last[s], {k: v[..., s:s + 1, :] for k, v in rec.items()}, (N, kernel, placement, s))
    eng.close()


def test_run_episode_takes_one_epsilon_per_scenario():
    N, R = 2, 1
    inp, lr, eps, *_ = _eps_reference(N, R, "f64", True)
    a, b = _device(inp, N, R, lr=lr), _device(inp, N, R, lr=lr)
    a.run_episode("train", "philox", episode=0, epsilon=eps[0], reset_sigma=0.3)
    b.run_episodes(0, eps[:1], reset_sigma=0.3)
    assert np.array_equal(a.get_q(), b.get_q()) and np.array_equal(a.episode_reward(), b.episode_reward())
    with pytest.raises(ValueError):
        a.run_episode("train", "philox", epsilon=eps[0, :3])
    with pytest.raises(ValueError):
        a.run_episode("greedy", epsilon=eps[0])
    with pytest.raises(ValueError):
        a.run_episodes(0, eps[:, :3])
    a.close()
    b.close()


# ----------------------------------------------------------------- 3. chains
def _state(eng):
    return (eng.get_q(), *eng.get_temperatures(), eng.episode_reward())


def _same_state(a, b):
    for x, y in zip(_state(a), _state(b)):
        assert np.array_equal(x, y)


def test_constant_rows_equal_run_episodes_and_leave_no_stale_prepass():
    N, R, n = 2, 1, 5
    inp = scenario_batch(S, N, T, seed=9)
    lr = _draw(S, N, seed=79)
    sched = np.array([0.81, 0.729, 0.5, 2.0 ** -10, 1.0])
    plain, table = _device(inp, N, R, lr=lr), _device(inp, N, R, lr=lr)
    # the plain context speculates episodes 5.. at `nxt`; the table call must leave no slot that a later
    # plain call at the same schedule could take as a hit
    nxt = np.array([0.3, 0.2, 0.1])
    plain.run_episodes(0, sched, reset_sigma=0.3, next_epsilons=nxt, record=REC)
    table.run_episodes(0, np.repeat(sched[:, None], S, axis=1), reset_sigma=0.3, record=REC)
    assert table.last_kernel() == plain.last_kernel()
    assert np.array_equal(table.episode_rewards(), plain.episode_rewards())
    _same_state(plain, table)
    ra, rb = plain.get_records(REC), table.get_records(REC)
    for k in REC:
        assert np.array_equal(ra[k], rb[k]), k
    # a plain call right after a table call: `plain` holds a speculated slot for (episode 5, nxt), the
    # table call at episode 5 overwrites it with its own words, and the plain calls that follow must
    # compute theirs again: they equal the same calls on a context that never made a table call
    mixed = np.random.RandomState(1).choice(EPS_VALUES, (3, S))
    q5 = plain.get_q()
    plain.set_temperatures(lr[3], lr[3])
    plain.run_episodes(5, mixed, reset_sigma=0.3)
    fresh = _device(inp, N, R, lr=lr)
    for eng in (plain, fresh):
        eng.set_q(q5)
        eng.set_temperatures(lr[3], lr[3])
        eng.run_episodes(5, nxt, reset_sigma=0.3)
    _same_state(fresh, plain)
    assert np.array_equal(fresh.episode_rewards(), plain.episode_rewards())
    for eng in (plain, fresh):
        eng.run_episodes(8, nxt, reset_sigma=0.3)
    _same_state(fresh, plain)
    for eng in (plain, table, fresh):
        eng.close()


def test_70_episode_table_call_equals_single_episode_calls():
    S4, N, R, T12, n = 4, 2, 1, 12, 70
    inp = scenario_batch(S4, N, T12, seed=61)
    lr = _draw(S4, N, seed=80)
    eps = np.random.RandomState(2).choice(EPS_VALUES, (n, S4))
    one, many = _device(inp, N, R, lr=lr), _device(inp, N, R, lr=lr)
    one.run_episodes(0, eps, reset_sigma=0.3)
    rew = []
    for k in range(n):
        many.run_episodes(k, eps[k:k + 1], reset_sigma=0.3)
        rew.append(many.episode_rewards()[0])
    assert np.array_equal(one.episode_rewards(), np.stack(rew))
    _same_state(one, many)
    one.close()
    many.close()


def test_interleaved_chain_with_arrays_and_table():
    """The shape tests/test_gpu_chain_interleave.py interleaves (S = 20, N = 2, T = 12 over a whole day)."""
    S20, N, R, T12, n = 20, 2, 1, 12, 6
    inp = scenario_batch(S20, N, T12, seed=61)
    inp = dataclasses.replace(inp, time=np.asarray(np.arange(T12) / float(T12), F32))
    lr = _draw(S20, N, seed=81)
    lr = lr[:3] + (inp.t_in0,)
    eps = np.random.RandomState(4).choice(EPS_VALUES, (n, S20))
    chain, single = _device(inp, N, R, lr=lr), _device(inp, N, R, lr=lr)
    chain.run_episodes(2, eps, reset_sigma=0.3, record=REC)
    assert ",interleaved" in chain.last_kernel(), chain.last_kernel()
    rew = []
    for k in range(n):
        single.run_episode("train", "philox", episode=2 + k, epsilon=eps[k], reset_sigma=0.3, record=REC)
        assert ",interleaved" not in single.last_kernel()
        rew.append(single.episode_reward())
    assert np.array_equal(chain.episode_rewards(), np.stack(rew))
    _same_state(chain, single)
    ra, rb = chain.get_records(REC), single.get_records(REC)
    for k in REC:
        assert np.array_equal(ra[k], rb[k]), k
    chain.close()
    single.close()


# ----------------------------------------------------------------- 4. sq16 hand-over
def test_sq16_hands_over_to_the_general_kernel_and_back():
    N, R = 16, 1
    inp = scenario_batch(S, N, T, seed=11)

    def run(eng):
        eng.zero_q()
        eng.set_temperatures(inp.t_in0, inp.t_m0)
        eng.run_episode("train", "philox", episode=0, epsilon=0.6, record=REC)
        return eng.last_kernel(), eng.get_records(REC), eng.get_q_delta()

    eng = _device(inp, N, R, "f32", shared_q=True)
    name0, rec0, d0 = run(eng)
    assert name0.startswith("episode_sq16_kernel<"), name0
    cfg = eng.cfg
    eng.set_learning(cfg.alpha, cfg.gamma, cfg.penalty_weight)  # the config's own values, uploaded
    name1, rec1, d1 = run(eng)
    assert name1.startswith("episode_kernel<"), name1
    for k in REC:
        assert np.array_equal(rec0[k], rec1[k]), k
    assert np.array_equal(d0, d1)
    eng.set_learning()
    name2, rec2, d2 = run(eng)
    assert name2.startswith("episode_sq16_kernel<"), name2
    assert np.array_equal(d0, d2)
    eng.run_episodes(0, np.full((1, S), 0.6))  # a table call: the general kernel's shared-table form
    assert eng.last_kernel().startswith("episode_kernel<"), eng.last_kernel()
    eng.close()


# ----------------------------------------------------------------- 5. defaults, validation, per-call use
def test_defaults_and_validation():
    S3, N = 3, 4
    inp = scenario_batch(S3, N, 8, seed=1)
    eng = _device(inp, N, 1)
    fresh = eng.get_learning()
    assert fresh["alpha"].shape == (S3, N) and fresh["penalty_weight"].dtype == F32
    assert np.all(fresh["alpha"] == eng.cfg.alpha) and np.all(fresh["gamma"] == eng.cfg.gamma)
    assert np.all(fresh["penalty_weight"] == F32(eng.cfg.penalty_weight))
    alpha, gamma, pen, _ = _draw(S3, N)
    eng.set_learning(alpha, gamma, pen)
    eng.set_learning(gamma=0.25)  # scalars broadcast; the fields left out go back to the config's
    got = eng.get_learning()
    assert np.all(got["gamma"] == 0.25) and np.array_equal(got["alpha"], fresh["alpha"])
    eng.set_learning(alpha, gamma, pen)
    before = eng.get_learning()

    def unchanged():
        now = eng.get_learning()
        return all(np.array_equal(now[k], before[k]) for k in before)

    def bad(x, v):
        y = np.array(x, copy=True)
        y[1, 2] = v
        return y
    for kw in (dict(alpha=bad(alpha, np.nan)), dict(alpha=bad(alpha, -1e-3)), dict(gamma=bad(gamma, 1.5)),
               dict(penalty_weight=bad(pen, -1.0)), dict(alpha=bad(alpha, 1.5)), dict(penalty_weight=bad(pen, np.inf))):
        with pytest.raises(_lib.P2PMGError, match="INVALID"):
            eng.set_learning(**{**dict(alpha=alpha, gamma=gamma, penalty_weight=pen), **kw})
        assert unchanged()
    eps = np.full((2, S3), 0.5)
    for v in (1.5, -0.1, np.nan):
        wrong = eps.copy()
        wrong[1, 2] = v
        with pytest.raises(_lib.P2PMGError, match="INVALID"):
            eng.run_episodes(0, wrong)
    L = eng.L
    import ctypes as C
    for mode, rng in ((_lib.MODE_GREEDY, _lib.RNG_PHILOX), (_lib.MODE_TRAIN, _lib.RNG_REPLAY)):
        args = _lib.EpisodeArgs(mode, rng, 0, 0, 0.5, 0, 0, 0.0, 0.0)
        assert L.p2pmg_run_episodes_eps(eng._ctx, C.byref(args), 2, eps) == 1  # P2PMG_E_INVALID
    assert unchanged()
    eng.set_learning()
    now = eng.get_learning()
    assert all(np.array_equal(now[k], fresh[k]) for k in fresh)
    eng.close()
    dqn = DeviceDQNBatch(1, 2, 1, 8, init_seed=1)
    a = np.full(2, 0.5)
    assert dqn.L.p2pmg_set_learning(dqn._ctx, a.ctypes.data, None, None) == 5  # P2PMG_E_UNSUPPORTED
    dqn.close()


def test_q_calls_train_with_each_agents_alpha_and_gamma():
    """QActor.train rl.py:125-128 in f64, in NumPy: q[s, a] += alpha ((r + gamma max q[ns]) - q[s, a])."""
    eng = DeviceCommunityBatch(1, 2, 0, 1)
    alpha, gamma = np.array([[0.1, 0.5]]), np.array([[0.3, 0.99]])
    eng.set_learning(alpha, gamma)
    rs = np.random.RandomState(0)
    tables = rs.uniform(-1, 1, (2, 20, 20, 20, 20, 3))
    eng.set_q(tables)
    n = 40
    agents = rs.randint(0, 2, n)
    s_obs = rs.uniform(-1, 1, (n, 4)).astype(F32)
    ns_obs = rs.uniform(-1, 1, (n, 4)).astype(F32)
    s_obs[:, 0], ns_obs[:, 0] = rs.uniform(0, 1, n), rs.uniform(0, 1, n)
    acts = rs.randint(0, 3, n)
    rewards = rs.uniform(-5, 0, n).astype(F32)
    eng.q_calls(agents, s_obs, acts, rewards=rewards, ns_obs=ns_obs, train=True)
    si, ni = eng.state_indices(s_obs), eng.state_indices(ns_obs)
    want = tables.copy()
    for k in range(n):
        q = want[agents[k]]
        s, ns, a = tuple(si[k]), tuple(ni[k]), acts[k]
        q[s][a] = q[s][a] + alpha[0, agents[k]] * ((np.float64(rewards[k]) + gamma[0, agents[k]] * np.max(q[ns])) - q[s][a])
    assert np.array_equal(eng.get_q(), want)
    assert not np.array_equal(want, tables)
    eng.close()
