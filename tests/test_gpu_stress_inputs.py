"""The episode kernels on inputs outside their fast-path domains (stress_cases.py) against the oracle, bit for
bit: Philox training, a replayed episode, a greedy day, under every kernel that serves the case.  The guards
and fallbacks each case reaches are proven on the oracle alone in test_cpu_stress_cases.py; here the kernels'
wiring of them (which lanes fall back, what a wave-uniform fallback does to the other lanes, the tot == 0
select after it, the hoisted reciprocal of a non-unit margin, the range-checked battery rule) must give the
oracle's records, rewards, temperatures, tables and SoC."""
from functools import lru_cache

import numpy as np
import pytest

import stress_cases as sc
from oracle.restatement import reference_replay_codes
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu
REC = sc.REC
EPS = 0.6


def _n_philox(c):
    return 1 if c.S * c.T * c.N > 3500 else 2  # one episode where S T N is largest


@lru_cache(maxsize=2)
def _reference(name, q_dtype):
    """The oracle's run of the case, once for every kernel and draw placement that is compared with it:
    a list of (what ran, its output, snapshots taken after it)."""
    c = sc.get(name)
    ob = sc.oracle_for(c, q_dtype)
    steps = []

    def snap(kind, out, codes=None):
        s = {"kind": kind, "out": out, "codes": codes, "soc": ob.soc.copy(), "t_in": ob.t_in.copy(), "t_m": ob.t_m.copy()}
        if c.shared and kind != "greedy":
            s["delta"] = ob.q_delta.copy()
            ob.apply_q_delta()
            s["q"] = ob.q.copy()
        steps.append(s)

    with np.errstate(all="ignore"):
        for e in range(_n_philox(c)):
            snap(("philox", e), ob.run_episode("train", rng="philox", seed=42, episode=e, eps=EPS))
        rss = [np.random.RandomState(42 + s) for s in range(c.S)]
        codes = np.stack([reference_replay_codes(rs, c.T, c.R, c.N, EPS) for rs in rss], axis=2)
        snap(("replay", 2), ob.run_episode("train", codes=codes, eps=EPS), codes)
        if c.codes is not None:  # the case's own replayed episode
            snap(("replay", 3), ob.run_episode("train", codes=c.codes, eps=EPS), c.codes)
        final_q = ob.q  # the greedy day leaves the tables as they are
        snap("greedy", ob.run_episode("greedy"))
    return steps, final_q


def _check_kernel(c, eng, kernel, placement):
    name = eng.last_kernel()
    if kernel == "general":
        assert name.startswith(f"episode_kernel<{c.N},") and "tile" not in name, name
    elif kernel == "tile":
        assert name.startswith(f"episode_kernel<{c.N},tile"), name
    elif c.auto_kernel is not None:
        fast = c.auto_kernel.startswith("episode_fast")
        if fast and placement == "inkernel":  # in-kernel draws are the general kernel's
            assert name.startswith("episode_kernel<"), name
            return
        assert name.startswith(c.auto_kernel), (name, c.auto_kernel)
        if c.range_checked is not None:
            assert ("range-checked" in name) == c.range_checked, name


def _run_case(name, kernel, placement, q_dtype):
    c = sc.get(name)
    steps, final_q = _reference(name, q_dtype)
    eng = sc.engine_for(c, q_dtype)
    dt = np.float64 if q_dtype == "f64" else np.float32
    for s in steps:
        kind, out = s["kind"], s["out"]
        if kind == "greedy":
            eng.run_episode("greedy", record=REC, kernel=kernel)
        elif kind[0] == "philox":
            eng.run_episode("train", "philox", episode=kind[1], epsilon=EPS, record=REC, kernel=kernel, philox=placement)
        else:
            eng.set_replay_codes(s["codes"])
            eng.run_episode("train", "replay", episode=kind[1], epsilon=EPS, record=REC, kernel=kernel)
        _check_kernel(c, eng, kernel, placement if kind != "greedy" and kind[0] == "philox" else "auto")
        tag = (name, kernel, placement, q_dtype, kind)
        _compare(out, eng.get_records(REC), tag)
        assert np.array_equal(eng.episode_reward(), out["episode_reward"]), tag
        a, b = eng.get_temperatures()
        assert np.array_equal(a, s["t_in"]) and np.array_equal(b, s["t_m"]), tag
        if c.capacity is not None:
            assert np.array_equal(eng.get_soc(), s["soc"]), tag
        if "delta" in s:
            assert np.array_equal(eng.get_q_delta().reshape(-1, 3), s["delta"]), tag
            eng.apply_q_delta()
            assert np.array_equal(eng.get_q(dtype=dt).reshape(s["q"].shape), s["q"]), tag
    assert np.array_equal(eng.get_q(dtype=dt).reshape(final_q.shape), final_q), (name, kernel, "tables")
    eng.close()


def _params():
    """(case, kernel, placement, q_dtype), a case's runs next to each other (they share one oracle run)."""
    out = []
    for name in sc.case_names():
        c = sc.get(name)
        kernels = ("auto", "general") if c.shared else ("auto", "general", "tile")
        if not (c.N <= 8 or c.N == 16):  # every other size runs the tile form, asked for or not
            kernels = ("auto", "tile")
        placements = ("prepass", "inkernel") if c.family in ("ladder", "zeros") else ("auto",)
        dtypes = ("f64", "f32") if c.family == "ladder" else (("f32",) if c.shared else ("f64",))
        for q in dtypes:
            for k in kernels:
                for pl in placements:
                    out.append(pytest.param(name, k, pl, q, id=f"{name}-{k}-{pl}-{q}"))
    return out


@pytest.mark.parametrize("name,kernel,placement,q_dtype", _params())
def test_stress_case_matches_oracle(name, kernel, placement, q_dtype):
    _run_case(name, kernel, placement, q_dtype)


CHAINED = ["ladder-agent4-one-k20", "ladder-agent2-one-k47", "onesided-agent4-r2", "onesided-agent2-r1",
           "lone-agent4-r2", "lone-agent2-r1"]


@pytest.mark.parametrize("name", CHAINED)
def test_chained_stress_case_matches_oracle(name):
    """8 chained episodes with the T0 reset (the pre-pass words, and at N = 2 the interleaved groups, on
    out-of-range lanes) against the oracle run episode by episode."""
    from test_gpu_chain_quad import E0, SIGMA, WIDE, _against_oracle, _schedule, _state
    c = sc.get(name)
    eng = sc.engine_for(c, "f64")
    eng.run_episodes(E0, _schedule(E0, 8), reset_sigma=SIGMA, record=WIDE)
    kernel, lag = eng.last_kernel(), eng.chain_lag()
    assert kernel.startswith("episode_fast_kernel<"), kernel
    if c.N == 2:  # the plan interleaves N = 2 chains only (p2pmg_plan.cpp)
        assert kernel.endswith(",interleaved>"), (kernel, lag)
    out = _state(eng, WIDE, np.float64)
    eng.close()
    with np.errstate(all="ignore"):
        _against_oracle(c, "f64", 8, out, r=c.R)
