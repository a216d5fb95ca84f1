"""Four chained episodes per wave, a quarter episode apart, as a NumPy model of the agents'
tables under the lockstep schedule (tests/quad_chain_ref.py), driven by access traces of oracle episodes.

The serial chain is nine oracle episodes (S = 20, N = 2, R = 0, T = 48, a 8 x 4 x 2 x 2 table, mostly
greedy) on a day whose steps 0 .. 7 share step 0's key: every store of those steps goes to a row the
wrap read of an earlier episode may need.  The model replays the traced accesses in the order four lane
groups run them (episode e in group e % 4, 12 steps behind e - 1) with the kernel's visibility: a load
sees another group's stores issued at least four lockstep steps before it for certain and later ones
perhaps (both must give the serial value), its own lane's last store through the patch, and the wrap
read takes the earliest follower's logged value.  The hazard distance of the day is D = 7 = T/4 - 5: the
model's four steps are counted from a store to the ISSUE of a load, one step ahead of the step that uses
it, so it holds one step below the kernel's rule D + 4 <= T/4 (which counts to the using step and rests
on a wave's accesses reaching the L1 in program order).
"""
import numpy as np
import pytest

from oracle import philox
import quad_chain_ref as ref
from test_gpu_wrap_log import S, N, SEED, _oracle, _shared_key_day

T, D_DAY, EPISODES, E0, SIGMA = 48, 7, 9, 2, 0.3
CFG = dict(n_time_states=8, n_temp_states=4, n_balance_states=2, n_p2p_states=2)


@pytest.fixture(scope="module")
def trace():
    inp = _shared_key_day(D_DAY, T=T, n_time=CFG["n_time_states"])
    ob = _oracle(inp, 0, "f64", **CFG)
    sp = np.full(S * N, float(ob.params.setpoint))

    def one(k):
        out = ob.run_episode("train", rng="philox", seed=SEED, episode=E0 + k, eps=0.1)
        t_in, t_m = philox.t0_draws(SEED, E0 + k + 1, np.arange(S * N), setpoint=sp, sigma=SIGMA)
        ob.t_in, ob.t_m = t_in.reshape(S, N), t_m.reshape(S, N)
        return out

    return ref.serial_traces(ob, one, EPISODES)


def test_day_is_inside_the_quarter_rule(trace):
    D = ref.hazard_distance(trace["lo"])
    assert D == D_DAY and D + 4 <= T // 4


def test_trace_holds_every_wrap_source(trace):
    """The oracle alone: wrap reads served by the loaded row, by e + 1's, e + 2's and e + 3's log."""
    counts = ref.wrap_sources(trace)
    print("wrap reads by source (loaded row, log of e + 1, e + 2, e + 3):", counts)
    assert counts.sum() == (EPISODES - 1) * S * N and (counts > 0).all(), counts


def test_quad_schedule_feeds_the_serial_values(trace):
    assert ref.lockstep_mismatches(trace, K=4, priority="earliest") == 0


def test_pair_schedule_feeds_the_serial_values(trace):
    """The two-group form on the same trace (its rule, e + 1's log or the loaded row, is complete there)."""
    assert ref.lockstep_mismatches(trace, K=2, priority="next") == 0


def test_two_group_priority_fails_for_four_groups(trace):
    """"e + 1's log or the loaded row" feeds a wrong TD target wherever only e + 2 or e + 3 stored into the row."""
    assert ref.lockstep_mismatches(trace, K=4, priority="next") > 0
