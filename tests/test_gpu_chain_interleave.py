"""Interleaved chained launches: episode e in lanes 0-31 of a wave and episode e + 1 of the same
agents in lanes 32-63, half an episode behind.  Every result must equal the same
episodes launched one by one, bit for bit: tables, temperatures, every episode's reward and the
last episode's records (narrow and wide).  Single launches never interleave, so they are the oracle.
The hazard distance the runtime decides by (p2pmg_chain_lag) is checked against a NumPy brute force
over the (time bin, balance bin) keys of the same observations.
"""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.engine import DeviceCommunityBatch

pytestmark = pytest.mark.gpu

WIDE = ("reward", "cost", "grid", "p2p", "t_in", "action", "index")
NARROW = ("reward", "cost")
F32 = np.float32


def _inputs(S, N, T, seed=61, time=None):
    """scenario_batch's day; below 96 steps the T steps span the whole day (a coarser slot), as the
    reference's one-day episode does, not the first T quarter hours of it."""
    inp = scenario_batch(S, N, T, seed=seed)
    if time is None and T != 96:
        time = np.arange(T) / float(T)
    return inp if time is None else dataclasses.replace(inp, time=np.asarray(time, F32))


def _engine(inp, N, R, q="f64", **cfg):
    S, T = inp.load_w.shape[0], inp.load_w.shape[-1]
    eng = DeviceCommunityBatch(S, N, R, T, q_dtype=q, **cfg)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    return eng


def _schedule(e0, n, floor=0.1):
    return [max(floor, 0.9 ** e) for e in range(e0, e0 + n)]


def _singles(eng, e0, eps, sigma, record):
    rew = []
    for k, e in enumerate(range(e0, e0 + len(eps))):
        eng.run_episode("train", "philox", episode=e, epsilon=eps[k], reset_sigma=sigma, record=record,
                        next_epsilon=eps[k + 1] if k + 1 < len(eps) else None)
        rew.append(eng.episode_reward())
    return np.stack(rew)


def _same(a, b, names):
    for x, y in zip(a.get_temperatures(), b.get_temperatures()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.episode_reward(), b.episode_reward())
    assert np.array_equal(a.get_q(), b.get_q())
    ra, rb = a.get_records(names), b.get_records(names)
    for k in names:
        assert np.array_equal(ra[k], rb[k]), k


def _check(inp, N, R, q, eps, e0=2, sigma=0.3, interleaved=True, **cfg):
    """The chain against single launches, once with wide and once with narrow records."""
    a = _engine(inp, N, R, q, **cfg)
    rew = _singles(a, e0, eps, sigma, WIDE)
    lag = None
    for names in (WIDE, NARROW):
        b = _engine(inp, N, R, q, **cfg)
        b.run_episodes(e0, eps, reset_sigma=sigma, record=names)
        name = b.last_kernel()
        assert name.startswith("episode_fast_kernel<"), name
        assert name.endswith(",interleaved>") == interleaved, name
        assert np.array_equal(b.episode_rewards(), rew)
        _same(a, b, names)
        lag = b.chain_lag()
        b.close()
    a.close()
    return lag


# ------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("T", [96, 24, 12])
@pytest.mark.parametrize("n", [2, 5, 6])
def test_interleaved_chain_equals_single_launches(T, n):
    _check(_inputs(20, 2, T), 2, 1, "f64", _schedule(2, n))


@pytest.mark.parametrize("S,R,q", [(33, 1, "f64"), (20, 1, "f32"), (20, 0, "f64")])
def test_interleaved_chain_other_shapes(S, R, q):
    """S no multiple of the scenarios per wave; an f32 table; R = 0 (one round, no candidate rows)."""
    _check(_inputs(S, 2, 96), 2, R, q, _schedule(2, 5))


def test_interleaved_70_episode_call_splits_64_plus_6():
    _check(_inputs(20, 2, 12), 2, 1, "f64", _schedule(0, 70), e0=0)


# -------------------------------------------------------------- 2. dense row collisions on the wrap
@pytest.mark.parametrize("R", [0, 1])
def test_dense_collisions_on_the_wrap(R):
    """A 6 x 2 x 2 x 2 table, mostly greedy: both episodes of a wave hit the same few rows all the
    time, and step T - 1's next-state rows (key of step 0) are rows the follower episode has been
    writing since its own step 0.  The LDS snapshot is what keeps the leader's TD target exact.
    R = 0 is the case that needs it: every TD store then goes to a p2p = 0 row, the kind the next-state
    rows are (at R = 1 the night-time stores go to the other p2p bin and the two sets stay apart).
    With the snapshot select compiled out (P2PMG_ABLATE=12) the R = 0 case fails."""
    cfg = dict(n_time_states=6, n_temp_states=2, n_balance_states=2, n_p2p_states=2)
    D, safe = _check(_inputs(20, 2, 48, time=np.arange(48) / 96.0), 2, R, "f64", [0.1] * 6, **cfg)
    assert safe and D + 4 <= 24, D


# --------------------------------------------------------------------------------- 3. refusals
def test_refused_equal_keys():
    """Constant profiles and a constant time column: every step has the same key (D = T - 1)."""
    inp = _inputs(20, 2, 24, time=np.full(24, 0.25))
    load = np.broadcast_to((0.3 * inp.max_in)[..., None], inp.load_w.shape).astype(F32)
    inp = dataclasses.replace(inp, load_w=np.ascontiguousarray(load), pv_w=np.zeros_like(load))
    D, safe = _check(inp, 2, 1, "f64", _schedule(2, 5), interleaved=False)
    assert (D, safe) == (23, False)


def test_refused_horizon_not_a_multiple_of_six():
    _check(_inputs(20, 2, 10), 2, 1, "f64", _schedule(2, 5), interleaved=False)


def test_refused_without_reset():
    _check(_inputs(20, 2, 24), 2, 1, "f64", _schedule(2, 5), sigma=None, interleaved=False)


_CHILD = """
import numpy as np
import test_gpu_chain_interleave as m
D, safe = m._check(m._inputs(20, 2, 24), 2, 1, "f64", m._schedule(2, 5), interleaved=False)
assert safe, D
print("child ok")
"""


def test_refused_by_environment_override():
    """P2PMG_INTERLEAVE=0 (read once per process): the serial chain, although the launch is safe."""
    env = dict(os.environ, P2PMG_INTERLEAVE="0")
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(os.path.abspath(__file__)),
                                         os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                         env.get("PYTHONPATH", "")])
    out = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------- 4. hazard distance
def _keys(eng, inp):
    """lo[a, t]: step t's (time bin, balance bin) of agent a; hi: the next step's, wrapping at T."""
    S, N, T = inp.load_w.shape
    bal = (inp.load_w - inp.pv_w) / inp.max_in[..., None]  # f32, as the step pre-pass computes it
    obs = np.zeros((S, N, T, 4), F32)
    obs[..., 0] = inp.time
    obs[..., 2] = bal
    idx = eng.state_indices(obs)
    lo = (idx[..., 0].astype(np.int64) * 65536 + idx[..., 2]).reshape(S * N, T)
    return lo, np.roll(lo, -1, axis=1)


def _lag(lo, hi):
    """max u - v over steps u of the earlier and v of the later episode that touch one key, a write
    involved: lo-lo, lo-hi, hi-lo.  Step T - 1's next-state read alone (hi(T - 1) = lo(0) against
    lo(v)) does not count: the snapshot serves it."""
    T = lo.shape[1]
    ll = lo[:, :, None] == lo[:, None, :]  # [a, u, v]
    lh = lo[:, :, None] == hi[:, None, :]
    hl = hi[:, :, None] == lo[:, None, :]
    hl[:, T - 1, :] = False
    c = (ll | lh | hl).any(axis=0)
    u, v = np.nonzero(c)
    return int((u - v).max())


def _planted(d):
    """T = 24 with one time bin per step, constant balances, and step 2 + d given step 2's time: the
    only keys that meet are d apart (lo-lo), d + 1 through the later episode's next-state row."""
    T = 24
    time = (np.arange(T) + 0.5) / T
    time[2 + d] = time[2]
    inp = _inputs(20, 2, T, time=time)
    load = np.broadcast_to((0.3 * inp.max_in)[..., None], inp.load_w.shape).astype(F32)
    return dataclasses.replace(inp, load_w=np.ascontiguousarray(load), pv_w=np.zeros_like(load))


@pytest.mark.parametrize("d,accepted", [(7, True), (8, False)])
def test_hazard_distance_at_the_threshold(d, accepted):
    """D + 4 = T / 2 exactly is accepted, D + 4 = T / 2 + 1 refused."""
    inp = _planted(d)
    D, safe = _check(inp, 2, 1, "f64", _schedule(2, 4), interleaved=accepted, n_time_states=24)
    eng = _engine(inp, 2, 1, n_time_states=24)
    assert D == _lag(*_keys(eng, inp)) == d + 1
    assert D + 4 == 12 + (0 if accepted else 1) and safe == accepted
    eng.close()


@pytest.mark.parametrize("T", [96, 24])
def test_hazard_distance_equals_brute_force(T):
    inp = _inputs(20, 2, T) if T == 96 else scenario_batch(20, 2, T, seed=61)  # T = 24: the first six hours
    eng = _engine(inp, 2, 1)
    eng.run_episodes(0, [0.5, 0.5], reset_sigma=0.3)
    D, safe = eng.chain_lag()
    assert D == _lag(*_keys(eng, inp))
    assert safe == (D + 4 <= T // 2)
    eng.close()
