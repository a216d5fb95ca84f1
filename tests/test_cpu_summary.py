"""p2pmg_episode_summary without a GPU: the NumPy definition (tests/summary_ref.py) against a case
worked out by hand, the ABI surface, and the non-triviality of every input set the GPU tests use."""
import numpy as np
import pytest

import summary_cases
import summary_ref

F32 = np.float32


def test_reference_helper_on_a_hand_written_case():
    """2 agents, 3 steps, R = 0, comfort band [20, 22]; every value is exact in f32."""
    col = lambda a0, a1: np.array([[a0[t], a1[t]] for t in range(3)], F32)[:, None, :]  # noqa: E731  [T, 1, 2]
    out = {"cost": col([0.5, -0.25, 1.0], [0.0, 0.0, 0.125]),
           "reward": col([-0.5, 0.25, -11.0], [0.0, 0.0, -0.125]),
           "grid": col([100.0, -50.0, 0.0], [-200.0, 25.0, -0.5]),
           "p2p": col([-25.0, 0.0, 75.0], [25.0, 0.0, -75.0]),
           "t_in": col([19.0, 20.5, 22.5], [21.0, 21.0, 21.0]),
           "action": np.array([[1, 2], [0, 2], [2, 1]])[:, None, None, :]}  # [T, 1, 1, 2]
    levels = np.array([[[0.0, 1500.0, 3000.0], [0.0, 1000.0, 2000.0]]], F32)
    load = np.array([[[200.0, 300.0, 400.0], [10.0, 20.0, 30.0]]], F32)
    pv = np.array([[[1000.0, 50.0, 0.0], [500.0, 0.0, 100.0]]], F32)
    agent, scen = summary_ref.summary(out, levels, load, pv, F32(20.0), F32(22.0))
    # agent 0: power = 75, -50, 75 -> self-consumption 1000, 50 - 50, 0; d = 1.0, 0, 0.5
    want0 = [1.25, -11.25, 100.0, 50.0, 75.0, 25.0, 4500.0, 900.0, 1050.0, 1000.0, 1.5, 2.0, 19.0, 22.5, 100.0, 50.0]
    # agent 1: power = -175, 25, -75.5 -> self-consumption 325, 0, 24.5; always inside the band
    want1 = [0.125, -0.125, 25.0, 200.5, 25.0, 75.0, 5000.0, 60.0, 600.0, 349.5, 0.0, 0.0, 21.0, 21.0, 25.0, 200.0]
    assert agent.shape == (1, 2, 16) and agent.dtype == np.float64
    assert agent[0, 0].tolist() == want0
    assert agent[0, 1].tolist() == want1
    # community: G = -100, -25, -0.5: it never imports, and exports 100 W at most
    want_s = [a + b for a, b in zip(want0[:12], want1[:12])] + [19.0, 22.5, 0.0, 100.0]
    assert scen.shape == (1, 16) and scen[0].tolist() == want_s
    # without a reward record field 1 is 0 and nothing else moves
    agent_nr, scen_nr = summary_ref.summary(out, levels, load, pv, F32(20.0), F32(22.0), reward=False)
    assert np.all(agent_nr[..., 1] == 0) and scen_nr[0, 1] == 0
    assert np.array_equal(np.delete(agent_nr, 1, axis=-1), np.delete(agent, 1, axis=-1))
    assert summary_ref.FIELDS[9] == "self_consumption" and len(summary_ref.FIELDS) == 16


def test_sequential_f64_order_is_what_the_helper_computes():
    """The sum is sequential over t in f64 of f32 terms: not a pairwise (np.sum) or an f32 sum."""
    rs = np.random.RandomState(0)
    T = 257
    cost = (rs.standard_normal((T, 1, 1)) * 1e3).astype(F32)
    z = np.zeros((T, 1, 1), F32)
    out = {"cost": cost, "reward": z, "grid": z, "p2p": z, "t_in": z + F32(21), "action": np.zeros((T, 1, 1, 1), int)}
    agent, _ = summary_ref.summary(out, np.zeros((1, 1, 3), F32), np.zeros((1, 1, T), F32), np.zeros((1, 1, T), F32),
                                   F32(20), F32(22))
    acc = 0.0
    for t in range(T):
        acc = acc + float(cost[t, 0, 0])
    assert agent[0, 0, 0] == acc


def test_symbol_and_abi_version():
    from p2pmicrogrid_amd import _lib, engine
    lib = _lib.lib()
    assert hasattr(lib, "p2pmg_episode_summary") and "p2pmg_episode_summary" in _lib.EXPORTS
    assert lib.p2pmg_abi_version() == 9
    assert engine.SUMMARY_FIELDS == summary_ref.FIELDS
    assert set(engine.SUMMARY_RECORDS) == {"cost", "grid", "p2p", "t_in", "action"}


def test_null_context_is_invalid():
    from p2pmicrogrid_amd import _lib
    buf = np.zeros(16, np.float64)
    assert _lib.lib().p2pmg_episode_summary(None, buf.ctypes.data, buf.ctypes.data) == 1  # P2PMG_E_INVALID
    assert _lib.lib().p2pmg_episode_summary(None, None, None) == 1


@pytest.mark.parametrize("name", sorted(summary_cases.CASES))
def test_expected_arrays_are_non_trivial(name):
    """No column of the GPU comparison is vacuous on any input set."""
    e = summary_cases.expected(name)
    c, inp, ag, sc = e["case"], e["inp"], e["agent"], e["scenario"]
    f = {n: ag[..., k] for k, n in enumerate(summary_ref.FIELDS)}
    assert ag.shape == (c.S, c.N, 16) and sc.shape == (c.S, 16) and np.all(np.isfinite(ag)) and np.all(np.isfinite(sc))
    assert (f["discomfort_steps"] > 0).any() and (f["discomfort_deg"] > 0).any()
    assert (f["grid_export"] != 0).any() and (f["grid_import"] != 0).any()
    if c.N >= 2:  # one agent has no peers: its p2p power is 0 by construction
        assert (f["p2p_import"] != 0).any() and (f["p2p_export"] != 0).any()
    assert (f["self_consumption"] != f["pv"]).any()
    assert (f["cost"] != 0).any() and (f["load"] > 0).any() and (f["pv"] > 0).any()
    if c.kind == "rule":
        assert np.all(f["reward"] == 0)
        lv2 = 3000.0  # level 2 of the default heat pump: a rule agent is off or at full power
        assert (f["hp"] > 0).any() and np.all(f["hp"] % lv2 == 0)
    else:
        assert (f["reward"] != 0).any()
    if c.T > 1 and not (c.pumps and 0.0 in c.pumps):
        assert (f["hp"] > 0).any()
    if c.T > 1:
        assert (f["t_in_min"] < f["t_in_max"]).any()
    # the community's peaks are not the sum or the maximum of its agents' peaks when flows cancel
    assert (sc[:, 14] > 0).any() or (sc[:, 15] > 0).any()
    if c.N >= 2 and c.T > 1:
        assert not np.array_equal(sc[:, 15], ag[..., 15].sum(axis=1))
    if c.setpoints is not None:
        lower, upper = c.bounds()
        assert len(np.unique(lower)) >= 2
        # the per-agent bounds matter: the config's band gives other discomfort totals
        other, _ = summary_ref.summary(e["out"], c.hp_levels(), inp.load_w, inp.pv_w, F32(20.0), F32(22.0))
        assert not np.array_equal(other[..., 10], ag[..., 10])
