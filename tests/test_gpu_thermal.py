"""Per-agent comfort setpoint, heat-pump COP and size on the device (p2pmg_set_thermal,
p2pmg_set_hp_levels) against the oracle, bit for bit.

The oracle takes per-agent values as [S, N] arrays in OracleParams(setpoint=..., hp_cop=...) and
OracleBatch(hp_levels=...).  Every setpoint drawn here is exactly representable in f32, so the f64
T0 oracle (philox.t0_draws(setpoint=array)) equals the device's (double)(float)setpoint.  The
initial temperatures are setpoint + 0.8 randn, so steps fall inside and outside the comfort band
from step 0 on, and a kernel that ignored the per-agent array could not pass."""
import functools

import numpy as np
import pytest

from oracle import dqn as odqn
from oracle import philox
from oracle.restatement import OracleBatch, OracleParams, reference_replay_codes, temperature_step
from p2pmicrogrid_amd import _lib
from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.dqn import DeviceDQNBatch
from p2pmicrogrid_amd.engine import DeviceCommunityBatch, unpack_index
from p2pmicrogrid_amd.heating import gA

pytestmark = pytest.mark.gpu
F32 = np.float32
REC = ["reward", "cost", "grid", "p2p", "t_in", "action", "index"]
SETPOINTS = (19.5, 21.0, 22.0, 23.25)
COPS = (2.5, 3.0, 4.0)
MAX_POWERS = (2e3, 3e3, 5e3)


def _draw_thermal(S, N, seed=1234, max_power=None):
    """setpoint, cop [S, N] f64; levels [S, N, 3] f32 = f32(level * max_power); T0 [S, N] f32."""
    rs = np.random.RandomState(seed)
    sp = rs.choice(SETPOINTS, (S, N))
    cop = rs.choice(COPS, (S, N))
    mp = rs.choice(MAX_POWERS, (S, N)) if max_power is None else np.full((S, N), float(max_power))
    lv = np.stack([(l * mp).astype(F32) for l in (0.0, 0.5, 1.0)], axis=-1)
    t0 = (sp + 0.8 * rs.randn(S, N)).astype(F32)
    return sp, cop, lv, t0


def _oracle_for(inp, N, R, q_dtype="f64", thermal=None, **kw):
    S = inp.load_w.shape[0]
    if thermal is not None:
        sp, cop, lv, _ = thermal
        kw.update(params=OracleParams(setpoint=sp, hp_cop=cop), hp_levels=lv)
    return OracleBatch(S=S, N=N, R=R, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in,
                       env_time=inp.time[None], env_tout=inp.t_out, q_dtype=q_dtype, **kw)


def _device_for(inp, N, R, q_dtype="f64", thermal=None, **kw):
    S, T = inp.load_w.shape[0], inp.load_w.shape[-1]
    eng = DeviceCommunityBatch(S, N, R, T, q_dtype=q_dtype, **kw)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    if thermal is not None:
        sp, cop, lv, _ = thermal
        eng.set_hp_levels(lv)
        eng.set_thermal(sp, cop)
    return eng


def _compare(out, rec, tag):
    for k in ("reward", "cost", "grid", "p2p", "t_in"):
        assert np.array_equal(rec[k], out[k]), (tag, k)
    assert np.array_equal(rec["action"], out["action"].astype(np.uint8)), tag
    assert np.array_equal(unpack_index(rec["index"]), out["idx"]), tag


# ----------------------------------------------------------------- 1. replay training
EPS = (0.81, 0.3)


@functools.lru_cache(maxsize=None)
def _replay_reference(N, R, T, q_dtype):
    """The oracle's run for one shape, computed once and shared by the kernel forms: inputs, codes,
    per-episode outputs, the greedy day, the final tables.  Nothing downstream modifies it."""
    S = 64
    inp = scenario_batch(S, N, T, seed=7)
    th = _draw_thermal(S, N)
    sp, cop, lv, t0 = th
    ob = _oracle_for(inp, N, R, q_dtype, thermal=th)
    ob.t_in, ob.t_m = t0.copy(), t0.copy()
    plain = _oracle_for(inp, N, R, q_dtype)  # the default parameters on the same inputs and codes
    plain.t_in, plain.t_m = t0.copy(), t0.copy()
    rss = [np.random.RandomState(42 + s) for s in range(S)]
    codes, outs = [], []
    for e, eps in enumerate(EPS):
        c = np.stack([reference_replay_codes(rs, T, R, N, eps) for rs in rss], axis=2)
        codes.append(c)
        outs.append(ob.run_episode("train", codes=c, eps=eps))
        if e == 0:
            dflt = plain.run_episode("train", codes=c, eps=eps)
    greedy = ob.run_episode("greedy")
    # the per-agent values matter on these inputs, and both sides of the comfort band are visited
    o = outs[0]
    for k in ("reward", "t_in", "idx"):
        assert not np.array_equal(o[k], dflt[k]), k
    lower, upper = (sp - 1.0).astype(F32), (sp + 1.0).astype(F32)
    pen = (o["t_in"] < lower) | (o["t_in"] > upper)
    assert pen.any() and not pen.all()
    assert np.array_equal(pen, o["reward"] < -(o["cost"] + F32(5)))  # penalty >= 10 (agent.py:230)
    return inp, th, codes, outs, greedy, ob.q.copy()


# (N, R, T, q_dtype) x kernel: auto is the fast kernel for N <= 8, the general kernel's register form
# at N = 16 and its LDS-tile form at 12 and 33; general / tile force those forms where they differ
REPLAY_CASES = [
    (2, 1, 24, "f64", "auto"), (2, 1, 24, "f64", "general"), (2, 1, 24, "f64", "tile"),
    (5, 2, 16, "f32", "auto"), (5, 2, 16, "f32", "general"), (5, 2, 16, "f32", "tile"),
    (8, 1, 12, "f64", "auto"), (8, 1, 12, "f64", "general"),
    (16, 1, 12, "f64", "auto"), (16, 1, 12, "f64", "tile"),
    (12, 1, 12, "f64", "auto"),
    (33, 0, 8, "f32", "auto"),
]


@pytest.mark.parametrize("N,R,T,q_dtype,kernel", REPLAY_CASES)
def test_replay_training_matches_oracle(N, R, T, q_dtype, kernel):
    S = 64
    inp, th, codes, outs, greedy, q_final = _replay_reference(N, R, T, q_dtype)
    eng = _device_for(inp, N, R, q_dtype, thermal=th)
    eng.set_temperatures(th[3], th[3])
    for e, eps in enumerate(EPS):
        eng.set_replay_codes(codes[e])
        eng.run_episode("train", "replay", episode=e, epsilon=eps, record=REC, kernel=kernel)
        out = outs[e]
        _compare(out, eng.get_records(REC), (N, R, T, q_dtype, kernel, e))
        assert np.array_equal(eng.episode_reward(), out["episode_reward"])
        a, b = eng.get_temperatures()
        assert np.array_equal(a, out["t_in_final"]) and np.array_equal(b, out["t_m_final"])
    q = eng.get_q(dtype=np.float64 if q_dtype == "f64" else np.float32)
    assert np.array_equal(q.reshape(S * N, -1, 3), q_final)
    eng.run_episode("greedy", record=REC, kernel=kernel)
    _compare(greedy, eng.get_records(REC), "greedy")
    eng.close()


# ----------------------------------------------------------------- 2. Philox, fused T0 reset, chain
def test_philox_chain_and_t0_reset_match_oracle():
    S, N, R, T = 128, 2, 1, 24
    eps = [0.81, 0.729, 0.5]
    inp = scenario_batch(S, N, T, seed=3)
    th = _draw_thermal(S, N, seed=5)
    sp, _, _, t0 = th
    ids = np.arange(S * N)
    ob = _oracle_for(inp, N, R, thermal=th)
    ob.t_in, ob.t_m = t0.copy(), t0.copy()
    want = []
    for e, x in enumerate(eps):
        want.append(ob.run_episode("train", rng="philox", seed=42, episode=e, eps=x)["episode_reward"])
        t_in, t_m = philox.t0_draws(42, e + 1, ids, setpoint=sp.ravel(), sigma=0.3)
        ob.t_in, ob.t_m = t_in.reshape(S, N), t_m.reshape(S, N)
    want = np.stack(want)

    chained = _device_for(inp, N, R, thermal=th)
    chained.set_temperatures(t0, t0)
    chained.run_episodes(episode=0, epsilons=eps, reset_sigma=0.3)
    single = _device_for(inp, N, R, thermal=th)
    single.set_temperatures(t0, t0)
    got = []
    for e, x in enumerate(eps):
        single.run_episode("train", "philox", episode=e, epsilon=x)
        got.append(single.episode_reward())
        single.reset_temperatures_philox(e + 1, 0.3)
    assert np.array_equal(chained.episode_rewards(), want)
    assert np.array_equal(np.stack(got), want)
    for eng in (chained, single):
        assert np.array_equal(eng.get_q().reshape(S * N, -1, 3), ob.q)
        a, b = eng.get_temperatures()
        assert np.array_equal(a, ob.t_in) and np.array_equal(b, ob.t_m)
        eng.close()


# ----------------------------------------------------------------- 3. shared table
def test_shared_table_with_and_without_thermal():
    S, N, R, T = 32, 16, 1, 12
    inp = scenario_batch(S, N, T, seed=11)
    th = _draw_thermal(S, N, seed=6)
    t0 = th[3]
    rss = [np.random.RandomState(42 + s) for s in range(S)]
    codes = np.stack([reference_replay_codes(rs, T, R, N, 0.6) for rs in rss], axis=2)
    eng = _device_for(inp, N, R, thermal=th, shared_q=True)
    eng.set_replay_codes(codes)

    def run_and_check(ob, tag):
        ob.t_in, ob.t_m = t0.copy(), t0.copy()
        eng.set_temperatures(t0, t0)
        eng.run_episode("train", "replay", episode=0, epsilon=0.6, record=REC)
        _compare(ob.run_episode("train", codes=codes, eps=0.6), eng.get_records(REC), tag)
        assert np.array_equal(eng.get_q_delta().reshape(-1, 3), ob.q_delta), tag
        eng.apply_q_delta()
        ob.apply_q_delta()
        assert np.array_equal(eng.get_q().reshape(ob.q.shape), ob.q), tag

    run_and_check(_oracle_for(inp, N, R, thermal=th, shared_q=True), "per-agent")
    assert not eng.last_kernel().startswith("episode_sq16_kernel<"), eng.last_kernel()
    # back to the config's values on a fresh table: the default-parameter oracle's result
    eng.set_thermal(None)
    eng.set_hp_levels(np.broadcast_to(OracleParams().hp_levels, (S, N, 3)))
    eng.zero_q()
    run_and_check(_oracle_for(inp, N, R, shared_q=True), "defaults")
    eng.close()


# ----------------------------------------------------------------- 4. rule kernel
def test_rule_episode_matches_oracle():
    S, N, R, T = 16, 5, 0, 48
    inp = scenario_batch(S, N, T, seed=13)
    th = _draw_thermal(S, N, seed=8)
    sp = th[0]
    t0 = (sp - 1.2).astype(F32)  # below every agent's own lower bound: every pump starts on
    hp_on = np.zeros((S, N), F32)
    ob = _oracle_for(inp, N, R, thermal=th)
    ob.t_in, ob.t_m = t0.copy(), t0.copy()
    out = ob.run_rule_episode(hp_on.copy())
    eng = _device_for(inp, N, R, thermal=th)
    eng.set_temperatures(t0, t0)
    eng.set_hp_state(hp_on)
    rec = ("cost", "grid", "p2p", "t_in", "action")
    eng.run_rule_episode(record=rec)
    got = eng.get_records(rec)
    for k in ("cost", "grid", "p2p", "t_in"):
        assert np.array_equal(got[k], out[k]), k
    assert np.array_equal(got["action"][:, 0], (2 * out["on"]).astype(np.uint8))
    assert np.array_equal(eng.get_hp_state(), out["hp_on"].astype(F32))
    assert out["on"].any() and not out["on"].all()  # both thresholds were crossed
    a, b = eng.get_temperatures()
    assert np.array_equal(a, ob.t_in) and np.array_equal(b, ob.t_m)
    eng.close()


# ----------------------------------------------------------------- 5. DQN
def _eq(got, want, what):
    assert np.array_equal(np.asarray(got), np.asarray(want)), what


@pytest.mark.parametrize("S,N,shared", [(2, 3, True), (2, 2, False)])
def test_dqn_episodes_match_oracle(S, N, shared):
    """The shared network's MFMA act kernel and the per-agent networks' wave act kernel with
    per-agent setpoint and COP (uniform 5 kW pumps: the DQN oracle takes its levels from
    OracleParams.hp_max_power): fill, then training at epsilon 0.9."""
    R, T, apb = 1, 40, 2
    inp = scenario_batch(S, N, T)
    sp, cop, lv, t0 = _draw_thermal(S, N, seed=9, max_power=5e3)
    eng = DeviceDQNBatch(S, N, R, T, shared=shared, init_seed=5, agents_per_block=apb if shared else 0,
                         grad_segments=1)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_hp_levels(lv)
    eng.set_thermal(sp, cop)
    eng.set_temperatures(t0, t0)
    ob = odqn.OracleDQNBatch(S=S, N=N, R=R, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in,
                             env_time=inp.time[None], env_tout=inp.t_out, theta0=eng.get_weights("online"),
                             shared=shared, agents_per_block=apb, grad_segments=1,
                             params=OracleParams(setpoint=sp, hp_cop=cop, hp_max_power=5e3))
    ob.t_in, ob.t_m = t0.copy(), t0.copy()
    th0 = ob.theta.copy()
    names = ["reward", "cost", "grid", "p2p", "t_in", "action", "loss"]
    for ep, (mode, eps) in enumerate((("fill", 1.0), ("train", 0.9))):
        eng.run_episode(mode, "philox", episode=ep, epsilon=eps, record=names)
        out = ob.run_episode(mode, rng="philox", episode=ep, eps=eps)
        rec = eng.get_records(names[:6] + (["loss"] if mode == "train" else []))
        _eq(rec["action"], out["action"].astype(np.uint8), "action")
        for k in ("reward", "cost", "grid", "p2p", "t_in") + (("loss",) if mode == "train" else ()):
            _eq(rec[k], out[k], k)
        _eq(eng.episode_reward(), out["episode_reward"], "episode reward")
        buf, added = eng.get_buffer()
        _eq(added, ob.added.ravel(), "added")
        n = int(added.min())
        _eq(buf[:, :n], ob.buf.reshape(S * N, -1, 10)[:, :n], "replay rings")
        eng.reset_temperatures_philox(ep + 1)
        ob.t_in, ob.t_m = (x.reshape(S, N) for x in philox.t0_draws(42, ep + 1, np.arange(S * N), setpoint=sp.ravel()))
        a, b = eng.get_temperatures()
        _eq(a, ob.t_in, "T0 in")
        _eq(b, ob.t_m, "T0 mass")
    _eq(eng.get_weights("online"), ob.theta, "online")
    _eq(eng.get_weights("target"), ob.target, "target")
    _eq(eng.get_weights("adam_m"), ob.m, "adam_m")
    _eq(eng.get_weights("adam_v"), ob.v, "adam_v")
    assert not np.array_equal(ob.theta, th0)
    eng.close()


# ----------------------------------------------------------------- 6. primitive
def test_rc_step_with_cop_and_solar_gain():
    rs = np.random.RandomState(0)
    n = 2000
    t_out = rs.uniform(-10, 30, n).astype(F32)
    t_in = rs.uniform(15, 25, n).astype(F32)
    t_m = rs.uniform(15, 25, n).astype(F32)
    hp = rs.choice([0.0, 1000.0, 1500.0, 2500.0, 5000.0], n).astype(F32)
    cop = rs.choice(COPS, n)
    eng = DeviceCommunityBatch(1, 1, 0, 1)
    a, b = eng.rc_step(t_out, t_in, t_m, hp, cop=cop, solar_gain=F32(gA * 50))
    wa, wb = temperature_step(t_out, t_in, t_m, hp, OracleParams(hp_cop=cop, solar_rad=50))
    assert np.array_equal(a, wa) and np.array_equal(b, wb)
    # no COP array: the config's COP with the solar term; neither: p2pmg_rc_step's result
    a, b = eng.rc_step(t_out, t_in, t_m, hp, solar_gain=F32(gA * 50))
    wa, wb = temperature_step(t_out, t_in, t_m, hp, OracleParams(solar_rad=50))
    assert np.array_equal(a, wa) and np.array_equal(b, wb)
    a, b = eng.rc_step(t_out, t_in, t_m, hp)
    wa, wb = temperature_step(t_out, t_in, t_m, hp)
    assert np.array_equal(a, wa) and np.array_equal(b, wb)
    eng.close()


# ----------------------------------------------------------------- 7. validation and round trip
def test_set_thermal_validation_and_round_trip():
    S, N = 3, 4
    eng = DeviceCommunityBatch(S, N, 1, 8)
    fresh = eng.get_thermal()
    assert fresh.shape == (S, N, 4) and fresh.dtype == F32
    assert np.array_equal(fresh, np.broadcast_to(np.array([21, 20, 22, 3], F32), (S, N, 4)))
    sp, cop, _, _ = _draw_thermal(S, N)
    eng.set_thermal(sp, cop)
    want = np.stack([sp.astype(F32), (sp - 1.0).astype(F32), (sp + 1.0).astype(F32), cop.astype(F32)], axis=-1)
    assert np.array_equal(eng.get_thermal(), want)
    eng.set_thermal(21.3, 4.0, lower=20.0, upper=23.5)  # scalars broadcast; explicit bounds kept
    assert np.array_equal(eng.get_thermal(), np.broadcast_to(np.array([21.3, 20.0, 23.5, 4.0], F32), (S, N, 4)))
    before = eng.get_thermal()
    bad = sp.copy()
    bad[1, 2] = np.nan
    bad_cop = cop.copy()
    bad_cop[2, 3] = np.inf
    for kw in (dict(setpoint=bad, cop=cop), dict(setpoint=sp, cop=bad_cop),
               dict(setpoint=sp, cop=cop, lower=sp + 1.0, upper=sp - 1.0)):
        with pytest.raises(_lib.P2PMGError, match="E_INVALID|INVALID"):
            eng.set_thermal(**kw)
        assert np.array_equal(eng.get_thermal(), before)  # a rejected call changes nothing
    eng.set_thermal(None)
    assert np.array_equal(eng.get_thermal(), fresh)
    eng.close()
