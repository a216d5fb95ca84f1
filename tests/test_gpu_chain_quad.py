"""Four chained episodes per wave, a quarter episode apart (`K=4,interleaved` in last_kernel()).

Every comparison is bit for bit.  The serial chain (P2PMG_INTERLEAVE=0, read once per process) runs in ONE
child process for the whole module, which leaves its results in a file; the oracle runs where T <= 24.
T = 12 cannot run four groups (T/4 = 3 < D + 4 for every D): those cases assert the two-group form, which
the plan falls back to, and compare it the same way.
"""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import philox
from oracle.restatement import OracleBatch, OracleParams
import quad_chain_ref as ref
from test_gpu_chain_interleave import F32, NARROW, WIDE, _engine, _inputs, _planted, _schedule
from test_gpu_wrap_log import SEED, _shared_key_day

pytestmark = pytest.mark.gpu

N, R, E0, SIGMA = 2, 1, 2, 0.3
SHAPES = [(S, T) for S in (3, 8, 20) for T in (12, 24, 96)]
CHAINS = (4, 5, 6, 7, 9)
DENSE_CFG = dict(n_time_states=8, n_temp_states=4, n_balance_states=2, n_p2p_states=2)


def _state(eng, names, qt):
    """Everything a chained launch leaves: table, temperatures, every episode's reward, the last one's records."""
    out = {"q": eng.get_q(dtype=qt), "rewards": eng.episode_rewards(), "ep_reward": eng.episode_reward()}
    out["t_in"], out["t_m"] = eng.get_temperatures()
    rec = eng.get_records(names)
    out.update({"rec_" + k: rec[k] for k in names})
    return out


def _run_chain(inp, q, n, names, R=R, eps=None, **cfg):
    eng = _engine(inp, N, R, q, **cfg)
    eng.run_episodes(E0, _schedule(E0, n) if eps is None else eps, reset_sigma=SIGMA, record=names)
    out = _state(eng, names, np.float64 if q == "f64" else np.float32)
    name, lag = eng.last_kernel(), eng.chain_lag()
    eng.close()
    return out, name, lag


def _cases():
    """name -> (inputs, table dtype, chain length, record names, R, epsilons, config)"""
    c = {}
    for S, T in SHAPES:
        inp = _inputs(S, N, T)
        for q in ("f64", "f32"):
            for n in CHAINS:
                for names in (WIDE, NARROW):
                    c[f"par-{S}-{T}-{q}-{n}-{len(names)}"] = (inp, q, n, names, R, None, {})
    c["dense"] = (_shared_key_day(7, T=48, n_time=8), "f64", 9, WIDE, 0, [0.1] * 9, DENSE_CFG)
    for d in (1, 2):  # D = d + 1 (test_gpu_chain_interleave._planted): T/4 - 4 = 2 and T/4 - 3 = 3 at T = 24
        c[f"planted-{d}"] = (_planted(d), "f64", 6, WIDE, R, None, dict(n_time_states=24))
    return c


def _serial_all(path):
    """The child's job: every case as a serial chain."""
    res = {}
    for key, (inp, q, n, names, r, eps, cfg) in _cases().items():
        out, name, _ = _run_chain(inp, q, n, names, R=r, eps=eps, **cfg)
        assert "interleaved" not in name, name
        res.update({f"{key}/{k}": v for k, v in out.items()})
    np.savez(path, **res)


@pytest.fixture(scope="module")
def serial(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("quad") / "serial.npz")
    env = dict(os.environ, P2PMG_INTERLEAVE="0")
    here = os.path.dirname(os.path.abspath(__file__))
    env["PYTHONPATH"] = os.pathsep.join([here, os.path.dirname(here), env.get("PYTHONPATH", "")])
    code = f"import test_gpu_chain_quad as m; m._serial_all({path!r}); print('child ok')"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stdout + out.stderr
    return np.load(path)


def _compare(serial, key, out):
    for k, v in out.items():
        assert np.array_equal(v, serial[f"{key}/{k}"]), (key, k)


def _oracle_chain(inp, q, n, r=R, eps=None, **cfg):
    """inp: scenario_batch's inputs, or anything with their fields; the community size is the profiles', a
    time table may be [T] or [S, T], and per-agent heat-pump levels are taken where inp has them."""
    S, N, T = inp.load_w.shape
    par = OracleParams(n_time=cfg.get("n_time_states", 20), n_temp=cfg.get("n_temp_states", 20),
                       n_bal=cfg.get("n_balance_states", 20), n_p2p=cfg.get("n_p2p_states", 20))
    ob = OracleBatch(S=S, N=N, R=r, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in,
                     env_time=np.asarray(inp.time, F32).reshape(-1, T), env_tout=inp.t_out, q_dtype=q, params=par,
                     hp_levels=getattr(inp, "hp_levels", None))
    ob.t_in, ob.t_m = inp.t_in0.copy(), inp.t_m0.copy()
    eps = _schedule(E0, n) if eps is None else eps
    sp = np.full(S * N, float(par.setpoint))

    def one(k):
        out = ob.run_episode("train", rng="philox", seed=SEED, episode=E0 + k, eps=eps[k])
        t_in, t_m = philox.t0_draws(SEED, E0 + k + 1, np.arange(S * N), setpoint=sp, sigma=SIGMA)
        ob.t_in, ob.t_m = t_in.reshape(S, N), t_m.reshape(S, N)
        return out

    return ob, one


def _against_oracle(inp, q, n, out, r=R, eps=None, **cfg):
    ob, one = _oracle_chain(inp, q, n, r, eps, **cfg)
    outs = [one(k) for k in range(n)]
    assert np.array_equal(out["q"].reshape(ob.q.shape), ob.q)
    assert np.array_equal(out["rewards"], np.stack([o["episode_reward"] for o in outs]))
    assert np.array_equal(out["t_in"], ob.t_in) and np.array_equal(out["t_m"], ob.t_m)
    for k in ("reward", "cost"):
        assert np.array_equal(out["rec_" + k], outs[-1][k]), k


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("q", ["f64", "f32"])
@pytest.mark.parametrize("S,T", SHAPES)
def test_quad_chain_equals_the_serial_chain(serial, S, T, q):
    """S = 3, 8, 20: a partial wave, exactly one wave, three waves (8 scenarios per wave at K = 4);
    chains of 4 .. 9: every (n - 1) % 4, fill and drain as long as the body."""
    inp = _inputs(S, N, T)
    for n in CHAINS:
        for names in (WIDE, NARROW):
            out, name, (D, safe) = _run_chain(inp, q, n, names)
            K = 4 if D + 4 <= T // 4 else 2
            assert T == 12 or K == 4, (T, D)  # the days of T = 24 and 96 are inside the quarter rule
            assert name.startswith("episode_fast_kernel<") and name.endswith(f",K={K},interleaved>"), name
            _compare(serial, f"par-{S}-{T}-{q}-{n}-{len(names)}", out)
            if T <= 24 and names is WIDE and n in (4, 9):
                _against_oracle(inp, q, n, out)


# ------------------------------------------------------------------------- 2. wrap-log density
def test_dense_wrap_rows_take_every_source(serial):
    """The dense-collision day of test_gpu_wrap_log (steps 0 .. 7 on step 0's key, R = 0, mostly greedy) with
    four temperature bins and nine episodes: the oracle's trace shows wrap reads served by the loaded row
    and by the log of e + 1, e + 2 and e + 3; then the chain must still equal the serial chain and the oracle."""
    inp, q, n, names, r, eps, cfg = _cases()["dense"]
    ob, one = _oracle_chain(inp, q, n, r, eps, **cfg)
    tr = ref.serial_traces(ob, one, n)
    counts = ref.wrap_sources(tr)
    print("wrap reads by source (loaded row, log of e + 1, e + 2, e + 3):", counts)
    assert (counts > 0).all(), counts
    out, name, (D, safe) = _run_chain(inp, q, n, names, R=r, eps=eps, **cfg)
    assert name.endswith(",K=4,interleaved>") and D + 4 <= 12, (name, D)
    _compare(serial, "dense", out)
    assert np.array_equal(out["q"].reshape(ob.q.shape), ob.q)
    assert np.array_equal(out["t_in"], ob.t_in) and np.array_equal(out["t_m"], ob.t_m)


# --------------------------------------------------------------------------------- 3. threshold
@pytest.mark.parametrize("d,K", [(1, 4), (2, 2)])
def test_hazard_distance_at_the_quarter_threshold(serial, d, K):
    """T = 24: D = T/4 - 4 = 2 runs four groups, D = T/4 - 3 = 3 falls back to two; both match."""
    inp, q, n, names, r, eps, cfg = _cases()[f"planted-{d}"]
    out, name, (D, safe) = _run_chain(inp, q, n, names, **cfg)
    assert D == d + 1 and safe and (D + 4 <= 6) == (K == 4)
    assert name.endswith(f",K={K},interleaved>"), name
    _compare(serial, f"planted-{d}", out)
    _against_oracle(inp, q, n, out, **cfg)
