"""The stress inputs of stress_cases.py, proven on the oracle alone: every case is finite end to end, puts at
least FLOOR (step, round, agent) triples on the far side of each guard it is built to flip (and, where it is a
mixed case, as many ordinary ones into the same wave-sized group at the same step and round), and the bin-edge
cases hit both end bins and both sides of an interior boundary on all four state axes.  No GPU.

Run with -s to see, per case, the triples on each side of each guard."""
from functools import lru_cache

import numpy as np
import pytest

import stress_cases as sc

F32 = np.float32
AXES = ("time", "temp", "bal", "p2p")


@lru_cache(maxsize=None)
def _run(name):
    """Episode 0 (Philox, epsilon 0.6) of the case on the oracle with its trace; a shared table also runs
    episode 1 on the applied deltas (the sums below cover both)."""
    c = sc.get(name)
    ob = sc.oracle_for(c)
    trace = []
    with np.errstate(all="ignore"):
        out = ob.run_episode("train", rng="philox", episode=0, eps=0.6, trace=trace)
    deltas = []
    if c.shared:
        deltas.append((ob.q_delta.copy(), np.stack([x["td_delta"] for x in trace])))
        ob.apply_q_delta()
        tr1 = []
        with np.errstate(all="ignore"):
            ob.run_episode("train", rng="philox", episode=1, eps=0.6, trace=tr1)
        deltas.append((ob.q_delta.copy(), np.stack([x["td_delta"] for x in tr1])))
    return c, ob, out, trace, deltas


def test_trace_changes_no_result():
    c = sc.get("battery-agent4-domain")
    a, b = sc.oracle_for(c), sc.oracle_for(c)
    tr = []
    x = a.run_episode("train", rng="philox", episode=0, eps=0.6)
    y = b.run_episode("train", rng="philox", episode=0, eps=0.6, trace=tr)
    assert len(tr) == c.T and x.keys() == y.keys()
    for k in x:
        assert np.array_equal(x[k], y[k]), k
    assert np.array_equal(a.q, b.q) and np.array_equal(a.soc, b.soc)


def test_shapes_stay_small():
    for name in sc.case_names():
        c = sc.get(name)
        assert 8 <= c.T <= 24 and c.R in (0, 1, 2), name
        assert (5 <= c.S <= 12) if c.N > 8 else (40 <= c.S <= 72), name
        for x in (c.time, c.t_out, c.load_w, c.pv_w, c.max_in, c.hp_levels, c.t_in0, c.t_m0):
            assert x.dtype == np.float32 and np.isfinite(x).all(), name
        if c.family == "ladder":
            assert in_range_40(c.max_in), name


def in_range_40(x):
    return bool(sc.in40(x).all())


@pytest.mark.parametrize("name", sc.case_names())
def test_oracle_is_finite(name):
    """No NaN or inf in any record, table, temperature or SoC (the int64 cast of a NaN bin is undefined)."""
    c, ob, out, trace, deltas = _run(name)
    for k in ("reward", "cost", "grid", "p2p", "t_in", "t_m", "hp", "episode_reward", "t_in_final", "t_m_final"):
        assert np.isfinite(out[k]).all(), (name, k)
    assert np.isfinite(ob.q).all() and np.isfinite(ob.t_in).all() and np.isfinite(ob.t_m).all(), name
    assert np.isfinite(ob.soc).all(), name
    for k in ("out", "tot", "num", "p2p_num", "p2pf", "bal", "tnorm", "cost_num"):
        assert all(np.isfinite(x[k]).all() for x in trace), (name, k)
    power = max(float(np.abs(x["out"]).max()) for x in trace)
    assert power <= (sc.SHARED_POWER_CAP if c.shared else sc.AGENT_POWER_CAP), (name, power)
    for q_delta, td in deltas:
        # the shared table's int64 fixed-point deltas (include/p2pmg.h): the sum of the magnitudes of everything
        # an episode adds stays below 2^62, whatever the rows it lands in and the order of the adds
        assert np.isfinite(td).all() and float(np.abs(np.rint(td)).sum()) < 2.0 ** 62, name
        assert int(np.abs(q_delta).max()) < 2 ** 62, name


@pytest.mark.parametrize("name", sc.case_names())
def test_guards_are_reached(name):
    c, ob, out, trace, _ = _run(name)
    n = sc.counts(c, sc.predicates(c, trace))
    print(f"\n{name}: (far side, ordinary, ordinary beside a far-side one in its wave) " +
          " ".join(f"{k}={v}" for k, v in n.items()))
    for k in c.flips:
        assert n[k][0] >= sc.FLOOR, (name, k, n)
    for k in c.mixed:
        assert n[k][2] >= sc.FLOOR, (name, k, n)
    for k in c.holds:
        assert n[k][0] == 0 and n[k][1] >= sc.FLOOR, (name, k, n)
    if name == "ladder-shared16-ev0-all":  # ok_ev0 is false on all 64 lanes of every wave at every step
        far = sc.predicates(c, trace)["ev0_ok"][:, 0]
        assert far.all(), name
    if "lane" in c.marks:  # the single-agent ladder: the scaled agent itself is on the far side of its guard
        s, i = c.marks["lane"]
        far = sc.predicates(c, trace)[c.flips[0]][:, :, s, i]
        assert far.any(), name


def test_ok_ev0_alone_decides_beside_denormal_numerators():
    """ladder-shared16-ev0-denormal under its own replay codes: on every lane of every wave at every step the
    round-0 split is out of range 19 while the round-1 net power and tot are in range, so `ok_ev0` alone keeps
    the wave off the packed quotient; the consumers' numerators towards the tiny peers are denormals (below
    1.1754943508222875e-38 = 2^-126) with normal quotients, and every agent's p2p record is a non-zero sum of
    such quotients alone (below 2^-100 in magnitude), so their last bit is visible in a compared record."""
    c = sc.get("ladder-shared16-ev0-denormal")
    ob = sc.oracle_for(c)
    trace = []
    out = ob.run_episode("train", codes=c.codes, eps=0.6, trace=trace)
    for k in ("reward", "cost", "grid", "p2p"):
        assert np.isfinite(out[k]).all(), k
    p = sc.predicates(c, trace)
    assert p["ev0_ok"][:, 0].all() and not p["out19"][:, 1].any() and not p["rt_ok"][:, 1].any()
    num = np.stack([x["num"] for x in trace])[:, 1]  # [T, S, N, N]
    tot = np.stack([x["tot"] for x in trace])[:, 1]
    tiny = (num > 0) & (num < 1.1754943508222875e-38) & (tot != 0)[..., None]
    with np.errstate(all="ignore"):
        quot = np.where(tiny, num / np.where(tot == 0, F32(1), tot)[..., None], F32(1))
    assert (quot >= 1.1754943508222875e-38).all()  # normal quotients
    lanes = tiny.any(axis=-1)
    pp = np.abs(out["p2p"])
    visible = (pp > 0) & (pp < 2.0 ** -100)
    print(f"\ndenormal numerators {int(tiny.sum())} on {int(lanes.sum())} (step, agent) pairs; p2p records made of their "
          f"quotients alone: {int(visible.sum())} of {pp.size}")
    assert lanes.sum() >= sc.FLOOR and visible.all()


def test_every_fallback_has_a_case():
    """Every guard is flipped by some case under the kernel that owns it, and every kernel choice the
    families name is asked for."""
    flipped = {}
    for name in sc.case_names():
        c = sc.get(name)
        for k in c.flips:
            flipped.setdefault((k, c.shared), []).append(name)
    for key in (("in19", True), ("ev0_ok", True), ("out19", True), ("p2p_num_ok", True), ("cost_num_ok", True),
                ("p2p_num_ok", False), ("cost_num_ok", False),
                ("rt_ok", True), ("num_ok", True), ("tot_zero", True), ("margin_one", True),
                ("bat_x", True), ("bat_q1", True), ("bat_space", True),
                ("rt_ok", False), ("num_ok", False), ("tot_zero", False), ("margin_one", False),
                ("bat_x", False), ("bat_q1", False), ("bat_space", False)):
        assert flipped.get(key), key
    assert {sc.get(n).auto_kernel for n in sc.case_names("max_in")} == {"episode_kernel<"}
    assert {sc.get(n).range_checked for n in sc.case_names("battery")} == {True, False}
    assert {sc.get(n).margin for n in sc.case_names("margin")} == {0.5, 2.0, 3.0}


def _axis_values(c, out, trace):
    """axis -> (observation [T, R + 1, S, N] f32, bin [T, R + 1, S, N]): what QActor bins (rl.py:89-95)."""
    idx = out["idx"]
    T, R1 = idx.shape[0], idx.shape[1]
    per_step = lambda k: np.broadcast_to(np.stack([x[k] for x in trace])[:, None], idx.shape[:-1])
    obs = {"time": per_step("time"), "temp": np.broadcast_to(out["t_in"][:, None], idx.shape[:-1]), "bal": per_step("bal"),
           "p2p": np.stack([x["p2pf"] for x in trace])}
    return {a: (np.asarray(obs[a], F32), idx[..., j]) for j, a in enumerate(AXES)}


@pytest.mark.parametrize("name", sc.case_names("bins") + sc.case_names("margin"))
def test_every_bin_edge_is_hit(name):
    """Bins 0 and K - 1 of each axis occur, and on each axis two observations one f32 ulp apart fall into
    different bins: one value within an ulp of an interior boundary on each side of it."""
    c, ob, out, trace, _ = _run(name)
    for axis, (x, b) in _axis_values(c, out, trace).items():
        assert b.min() == 0 and b.max() == 19, (name, axis, b.min(), b.max())
        xs, first = np.unique(x.ravel(), return_index=True)
        bs = b.ravel()[first]
        assert all((b.ravel()[x.ravel() == v] == k).all() for v, k in zip(xs[:50], bs[:50]))  # one bin per value
        step = (np.nextafter(xs[:-1], F32(np.inf)) == xs[1:]) & (bs[:-1] != bs[1:])
        assert step.any(), (name, axis)
        print(f"\n{name} {axis}: {int(step.sum())} neighbouring pairs across a boundary, bins {sorted(set(bs[:-1][step]))}")


@pytest.mark.parametrize("name", sc.case_names("battery"))
def test_battery_marks(name):
    c, ob, out, trace, _ = _run(name)
    s, i = c.marks["zero_balance"]
    assert c.capacity[s, i] > 0
    assert all((x["energy"][:, s, i] == 0).all() and not x["dis"][:, s, i].any() and not x["chg"][:, s, i].any()
               for x in trace), name
    s, i = c.marks["energy_eq"]
    x = trace[0]
    assert x["dis"][0, s, i] and x["energy"][0, s, i] == x["avail_energy"][0, s, i] and x["energy"][0, s, i] > 0, name
    assert float(F32(c.load_w[s, i, 0])) * 900.0 == x["energy"][0, s, i]
    smin, smax, _ = c.bounds
    for v in (smin, smax, np.nextafter(smin, 0), np.nextafter(smin, 1), np.nextafter(smax, 0), np.nextafter(smax, 1), 0.0):
        assert (c.soc0 == v).any(), v
    caps = set(np.unique(c.capacity))
    want = {"domain": {2.0 ** -20, 2.0 ** 60}, "outside": {2.0 ** -20, 2.0 ** 60, 2.0 ** -21},
            "window": {2.0 ** -320, 2.0 ** 340}}[name.rsplit("-", 1)[1]]
    assert want <= caps, caps
