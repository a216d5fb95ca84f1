"""Per-role policy tables (``shared_q="role"``, P2PMG_SHARED_ROLE) on the device: N tables, agent
(s, i) of every scenario reads table i, TD deltas summed per role in int64 fixed point.

Expected values come from the per-agent oracle through tests/role_tables.py (frozen-table trick and
delta helper, checked against the oracle's own shared table in tests/test_cpu_role_tables.py).
Every comparison is exact.  S = 7 scenarios fill waves partly and leave a last workgroup short."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.restatement import OracleParams, reference_replay_codes
from p2pmicrogrid_amd import _lib
from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.engine import DeviceCommunityBatch, unpack_index
from role_tables import applied, frozen_oracle, random_tables, role_deltas, set_role_tables

pytestmark = pytest.mark.gpu
F32 = np.float32
REC = ["reward", "cost", "grid", "p2p", "t_in", "action", "index"]
S, T = 7, 12


def _np_dtype(q_dtype):
    return np.float64 if q_dtype == "f64" else np.float32


def _device(inp, N, R, q_dtype="f64", shared_q="role", **kw):
    eng = DeviceCommunityBatch(inp.load_w.shape[0], N, R, inp.load_w.shape[-1], q_dtype=q_dtype, shared_q=shared_q, **kw)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    return eng


def _same(out, eng, tag):
    """records, final temperatures and episode reward of the last launch against an oracle episode"""
    rec = eng.get_records(REC)
    for k in ("reward", "cost", "grid", "p2p", "t_in"):
        assert np.array_equal(rec[k], out[k]), (tag, k)
    assert np.array_equal(rec["action"], out["action"].astype(np.uint8)), tag
    assert np.array_equal(unpack_index(rec["index"]), out["idx"]), tag
    a, b = eng.get_temperatures()
    assert np.array_equal(a, out["t_in_final"]) and np.array_equal(b, out["t_m_final"]), tag
    assert np.array_equal(eng.episode_reward(), out["episode_reward"]), tag
    return rec


def _role_kernel(eng, N, tile=False):
    k = eng.last_kernel()
    assert k.startswith(f"episode_kernel<{N},") and ",shared,roles" in k, k
    assert ("tile" in k) == tile, k


# ----------------------------------------------------------------- 1. greedy
@functools.lru_cache(maxsize=None)
def _greedy_reference(N, R):
    inp = scenario_batch(S, N, T, seed=7)
    tables = random_tables(N)
    return inp, tables, frozen_oracle(inp, N, R, tables).run_episode("greedy")


@pytest.mark.parametrize("R", [0, 2])
@pytest.mark.parametrize("N", [2, 3, 5, 8, 16, 12, 33])
def test_greedy_matches_oracle_and_per_agent_tables(N, R):
    inp, tables, out = _greedy_reference(N, R)
    eng = _device(inp, N, R)
    eng.set_q(tables)
    assert eng.get_q().shape == (N, 20, 20, 20, 20, 3)
    eng.run_episode("greedy", record=REC)
    _role_kernel(eng, N, tile=N in (12, 33))
    rec = _same(out, eng, ("role", N, R))
    # a shared_q = 0 context holding the replicated tables
    per = _device(inp, N, R, shared_q=False)
    per.set_q(np.tile(tables, (S, 1, 1)))
    per.run_episode("greedy", record=REC)
    got = per.get_records(REC)
    for k in REC:
        assert np.array_equal(got[k], rec[k]), ("per-agent", N, R, k)
    assert np.array_equal(per.episode_reward(), eng.episode_reward())
    per.close()
    if N <= 8:  # the same role context on the LDS-tile form
        eng.set_temperatures(inp.t_in0, inp.t_m0)
        eng.run_episode("greedy", record=REC, kernel="tile")
        _role_kernel(eng, N, tile=True)
        _same(out, eng, ("role-tile", N, R))
    assert np.array_equal(eng.get_q().reshape(tables.shape), tables)  # GREEDY only reads
    eng.close()


# ----------------------------------------------------------------- 2. train
EPS = (0.6, 0.3)


def _train_and_check(eng, ob, tables, run_dev, run_ora, tag):
    """two training episodes, each followed by apply_q_delta, then a greedy day"""
    dt = tables.dtype
    for e, eps in enumerate(EPS):
        run_dev(e, eps)
        out = run_ora(e, eps)
        _same(out, eng, (tag, e))
        assert np.array_equal(eng.get_q(dtype=dt).reshape(tables.shape), tables), (tag, e)  # frozen in the episode
        delta = role_deltas(ob, out, tables)
        assert np.count_nonzero(delta.reshape(ob.N, -1).any(axis=1)) == ob.N  # every role learned something
        assert np.array_equal(eng.get_q_delta().reshape(delta.shape), delta), (tag, e)
        eng.apply_q_delta()
        assert not eng.get_q_delta().any()
        tables = applied(tables, delta)
        assert np.array_equal(eng.get_q(dtype=dt).reshape(tables.shape), tables), (tag, e)
        set_role_tables(ob, tables)
    eng.run_episode("greedy", record=REC)
    _same(ob.run_episode("greedy"), eng, (tag, "greedy"))


@pytest.mark.parametrize("q_dtype", ["f64", "f32"])
@pytest.mark.parametrize("R", [0, 2])
@pytest.mark.parametrize("N", [2, 5, 12, 16])
def test_training_with_replay_codes(N, R, q_dtype):
    inp = scenario_batch(S, N, T, seed=7)
    tables = random_tables(N, q_dtype)
    ob = frozen_oracle(inp, N, R, tables, q_dtype)
    eng = _device(inp, N, R, q_dtype)
    eng.set_q(tables)
    rss = [np.random.RandomState(42 + s) for s in range(S)]
    codes = [np.stack([reference_replay_codes(rs, T, R, N, eps) for rs in rss], axis=2) for eps in EPS]

    def run_dev(e, eps):
        eng.set_replay_codes(codes[e])
        eng.run_episode("train", "replay", episode=e, epsilon=eps, record=REC)
        _role_kernel(eng, N, tile=N == 12)
    _train_and_check(eng, ob, tables, run_dev, lambda e, eps: ob.run_episode("train", codes=codes[e], eps=eps),
                     (N, R, q_dtype))
    eng.close()


@pytest.mark.parametrize("R", [0, 2])
def test_training_with_philox_draws(R):
    N = 2
    inp = scenario_batch(S, N, T, seed=7)
    tables = random_tables(N)
    ob = frozen_oracle(inp, N, R, tables)
    eng = _device(inp, N, R)
    eng.set_q(tables)
    _train_and_check(eng, ob, tables,
                     lambda e, eps: eng.run_episode("train", "philox", episode=e, epsilon=eps, record=REC),
                     lambda e, eps: ob.run_episode("train", rng="philox", episode=e, eps=eps), ("philox", R))
    eng.close()


# ----------------------------------------------------------------- 3. N = 1
def test_one_agent_is_the_shared_table():
    Sn, N, R = 64, 1, 1
    inp = scenario_batch(Sn, N, T, seed=7)
    tables = random_tables(N)
    a = _device(inp, N, R)
    b = _device(inp, N, R, shared_q=True)
    for eng in (a, b):
        eng.set_q(tables)
        eng.run_episode("train", "philox", episode=0, epsilon=0.5, record=REC)
    assert ",roles" in a.last_kernel() and ",roles" not in b.last_kernel() and ",shared" in b.last_kernel()
    ra, rb = a.get_records(REC), b.get_records(REC)
    for k in REC:
        assert np.array_equal(ra[k], rb[k]), k
    da, db = a.get_q_delta(), b.get_q_delta()
    assert da.shape == (1, 20, 20, 20, 20, 3) and db.shape == (20, 20, 20, 20, 3)
    assert db.any() and np.array_equal(da[0], db)
    a.apply_q_delta()
    b.apply_q_delta()
    assert np.array_equal(a.get_q(), b.get_q())
    a.close()
    b.close()


# ----------------------------------------------------------------- 4. split invariance
def test_scenario_split_does_not_change_the_tables():
    """S = 8 in one context = S = 5 plus S = 3 in two (scenario_offset, Philox draws by global agent
    id), their int64 deltas added on the host."""
    N, R = 3, 1
    inp = scenario_batch(8, N, T, seed=7)
    tables = random_tables(N)

    def part(lo, hi):
        import dataclasses
        sub = dataclasses.replace(inp, **{k: getattr(inp, k)[lo:hi]
                                          for k in ("load_w", "pv_w", "max_in", "t_in0", "t_m0", "t_out")})
        eng = _device(sub, N, R, scenario_offset=lo)
        eng.set_q(tables)
        eng.run_episode("train", "philox", episode=3, epsilon=0.5)
        return eng
    whole, first, second = part(0, 8), part(0, 5), part(5, 8)
    total = first.get_q_delta() + second.get_q_delta()
    assert total.any() and np.array_equal(total, whole.get_q_delta())
    whole.apply_q_delta()
    want = whole.get_q()
    assert not np.array_equal(want.reshape(tables.shape), tables)
    for eng in (first, second):
        eng.set_q_delta(total)
        eng.apply_q_delta()
        assert np.array_equal(eng.get_q(), want)
    for eng in (whole, first, second):
        eng.close()


# ----------------------------------------------------------------- 5. heterogeneous agents
def test_heterogeneous_agents_match_oracle():
    """per-agent heat-pump size (3 kW / 5 kW), setpoint (21 / 22) and battery, through set_hp_levels,
    set_thermal and set_battery as with one shared table"""
    Sn, N, R = 4, 3, 1
    inp = scenario_batch(Sn, N, T, seed=7)
    tables = random_tables(N)
    rs = np.random.RandomState(1)
    mp = rs.choice([3e3, 5e3], (Sn, N))
    lv = np.stack([(l * mp).astype(F32) for l in (0.0, 0.5, 1.0)], axis=-1)
    sp = rs.choice([21.0, 22.0], (Sn, N))
    cap = np.where(rs.rand(Sn, N) < 0.5, 10 * 3.6e6, 0.0)
    assert len(np.unique(mp)) == 2 and len(np.unique(sp)) == 2 and len(np.unique(cap)) == 2
    ob = frozen_oracle(inp, N, R, tables, params=OracleParams(setpoint=sp), hp_levels=lv, battery_capacity=cap)
    eng = _device(inp, N, R)
    eng.set_q(tables)
    eng.set_hp_levels(lv)
    eng.set_thermal(sp)
    eng.set_battery(cap, 0.1, 0.9, 0.9)
    eng.run_episode("train", "philox", episode=0, epsilon=0.5, record=REC)
    assert ",battery" in eng.last_kernel()
    _role_kernel(eng, N)
    out = ob.run_episode("train", rng="philox", episode=0, eps=0.5)
    _same(out, eng, "hetero-train")
    assert np.array_equal(eng.get_soc(), ob.soc)
    assert np.array_equal(eng.get_q_delta().reshape(tables.shape), role_deltas(ob, out, tables))
    eng.run_episode("greedy", record=REC)
    _same(ob.run_episode("greedy"), eng, "hetero-greedy")
    assert np.array_equal(eng.get_soc(), ob.soc)
    eng.close()


# ----------------------------------------------------------------- 6. refusals, unchanged dispatch
def test_refusals():
    L = _lib.lib()
    cfg = _lib.default_config()
    cfg.shared_q, cfg.learner = _lib.SHARED_ROLE, _lib.LEARNER_DQN
    ctx = C.c_void_p()
    assert L.p2pmg_create(C.byref(cfg), 0, C.byref(ctx)) == 5 and not ctx.value  # UNSUPPORTED
    with pytest.raises(_lib.P2PMGError, match="UNSUPPORTED.*P2PMG_SHARED_ROLE"):
        DeviceCommunityBatch(2, 2, 1, T, shared_q="role", learner=_lib.LEARNER_DQN)
    N = 3
    eng = DeviceCommunityBatch(4, N, 1, T, shared_q="role")
    one = np.zeros((1, 20 ** 4 * 3))
    eng.set_q(one, first=N - 1)
    for first, count in ((N, 1), (N - 1, 2), (0, N + 1)):
        with pytest.raises(_lib.P2PMGError, match="INVALID"):
            eng.set_q(np.repeat(one, count, axis=0), first=first)
        with pytest.raises(_lib.P2PMGError, match="INVALID"):
            eng.get_q(first=first, count=count)
    eng.close()


@pytest.mark.parametrize("N,shared,kernel", [
    (2, False, "episode_fast_kernel<2,f64,R1=2,greedy>"), (16, False, "episode_kernel<16,f64,R1=2>"),
    (2, True, "episode_kernel<2,f64,R1=2,shared>"), (16, True, "episode_sq16_kernel<16,f64,R1=2,greedy,shared>")])
def test_other_modes_report_the_kernels_they_did(N, shared, kernel):
    inp = scenario_batch(S, N, T, seed=7)
    eng = _device(inp, N, 1, shared_q=shared)
    eng.run_episode("greedy")
    assert eng.last_kernel() == kernel
    eng.close()
