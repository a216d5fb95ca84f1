"""CPU side of the shared-table TD-delta tests: the builders of shared_delta_cases.py meet the
preconditions that test_gpu_shared_delta.py asserts before it launches, window_keys restates the
oracle's delta keys, and the oracle's rounding is exact round-half-even.  A later edit of a builder
fails here, without a GPU."""
import functools

import numpy as np
import pytest

import shared_delta_cases as C
from oracle.restatement import DELTA_SCALE


@functools.lru_cache(maxsize=None)
def _crowded_first_episode(S, N, T):
    """The oracle's first episode (epsilon = 1, zero table) on the crowded builder, computed once per
    shape; nothing downstream modifies it."""
    inp = C.crowded_inputs(S, N, T, seed=5)
    ob = C.oracle_for(inp, 1)
    out = ob.run_episode("train", rng="philox", episode=0, eps=1.0)
    return inp, out, ob.q_delta.copy()


@functools.lru_cache(maxsize=None)
def _wide_first_episode(q_dtype="f32"):
    inp = C.wide_delta_inputs()
    ob = C.oracle_for(inp, 1, q_dtype, battery=False)
    out = ob.run_episode("train", rng="philox", episode=0, eps=0.6)
    return inp, ob, out, ob.q_delta.copy()


# ----------------------------------------------------------------------------- the builders
def test_crowded_builder_overfills_one_sq16_workgroup_and_not_the_other():
    """S = 40, T = 20: the full workgroup's windows of 8 steps hold well over 2048 distinct keys
    (measured 3522, 3542, and 1786 in the 4-step tail), the 8-scenario workgroup's stay below."""
    _, out, _ = _crowded_first_episode(40, 16, 20)
    full, part = C.workgroup_window_keys(out, C.SQ16_WG_SCENARIOS)
    assert len(full) == 3 and len(part) == 3
    assert min(full[:2]) >= 2300, full
    assert max(part) < C.HASH_SLOTS, part
    assert C.window_keys(out, 0, 32) == full and C.window_keys(out, 32, 8) == part


def test_crowded_builder_overfills_all_nine_workgroups():
    _, out, _ = _crowded_first_episode(288, 16, 12)
    counts = C.workgroup_window_keys(out, C.SQ16_WG_SCENARIOS)
    assert len(counts) == 9 and min(c[0] for c in counts) > C.HASH_SLOTS, counts


@pytest.mark.parametrize("N,S,spw,role", [(16, 35, 16, False), (12, 35, 16, False), (2, 259, 128, False),
                                          (4, 131, 64, False), (3, 131, 64, True)])
def test_crowded_builder_loads_the_general_forms_hash(N, S, spw, role):
    """256-lane workgroups: at most 2048 agent-steps per window, of which more than 1200 are distinct
    keys in both full workgroups (twice the ~600 of the benched inputs)."""
    _, out, _ = _crowded_first_episode(S, N, 20)
    counts = C.workgroup_window_keys(out, spw, role_keys=role)
    assert len(counts) == 3
    for c in counts[:2]:
        assert 1200 < max(c) <= C.HASH_SLOTS, counts


def test_crowded_builder_changes_the_time_bin_every_step():
    inp, _, _ = _crowded_first_episode(40, 16, 20)
    tbin = np.minimum((inp.time * np.float32(20)).astype(np.int64), 19)
    assert (tbin[:, 1:] != tbin[:, :-1]).all()
    assert (np.abs(inp.load_w - inp.pv_w) <= inp.max_in[..., None]).all()
    assert ((inp.load_w == 0) | (inp.pv_w == 0)).all()


def test_wide_builder_straddles_2_pow_51_wave_by_wave():
    inp, _, out, _ = _wide_first_episode()
    x = inp.alpha * out["reward"].astype(np.float64) * 2.0 ** 40
    below, above, mixed = C.wave_partition(x)
    assert below >= 1 and above >= 1 and mixed >= 1, (below, above, mixed)
    assert (below, above, mixed) == (64, 1, 7)  # the figures test_gpu_shared_delta.py quotes
    ax = np.abs(x)
    assert int(((x < 0) & (ax >= 2.0 ** 50) & (ax < 2.0 ** 51)).sum()) == 92
    assert ax.max() < 2.0 ** 57


def test_wide_builder_puts_negative_values_near_2_pow_51_in_a_wave_wholly_below_it():
    """Only a wave whose 64 lanes all lie below 2^51 takes sq16's two-instruction rounding: the values
    that try its high-word subtraction for a negative x close to -2^51 are those with |x| in
    [2^50, 2^51) in such a wave (wave 5 at step 0), not the ones beside a lane at or above 2^51."""
    inp, _, out, _ = _wide_first_episode()
    x = inp.alpha * out["reward"].astype(np.float64) * 2.0 ** 40
    assert C.fast_branch_negative_near_bound(x) == 9
    below = C.in_wave_below(x)
    assert below[0, 20:24].all() and not below[0, 4:20].any() and below[0, 0:4].all()
    w5 = np.abs(x[0, 20:24])
    assert 2.0 ** 50 < w5.max() < 2.0 ** 51 and (x[0, 20:24][w5 >= 2.0 ** 50] < 0).all()


def test_in_wave_below_marks_whole_waves():
    x = np.full((1, 8, 2), -2.0 ** 50)
    x[0, 5, 1] = 2.0 ** 51  # one lane of wave 1 at the bound: none of that wave's lanes counts
    m = C.in_wave_below(x)
    assert m[0, :4].all() and not m[0, 4:].any()
    assert C.fast_branch_negative_near_bound(x) == 8


def test_wide_builder_keeps_the_int64_sums_below_2_pow_62():
    """Python ints: the batch's sum of |delta| in episode 0, and every entry of the summed delta in the
    two episodes after it (table values of 1e5 in the targets)."""
    inp, _, out, _ = _wide_first_episode()
    assert sum(abs(int(v)) for v in C.first_episode_delta(out, inp.alpha).ravel()) < 2 ** 62
    ob = C.oracle_for(inp, 1, battery=False)
    for e in range(3):
        ob.run_episode("train", rng="philox", episode=e, eps=0.6)
        assert max(abs(int(v)) for v in ob.q_delta.ravel()) < 2 ** 62, e
        ob.apply_q_delta()


def test_wide_builder_stays_inside_the_range_free_division():
    inp, _, out, _ = _wide_first_episode()
    assert C.cost_operands_in_fast_range(out, inp)
    for x in inp.prices:  # exact power-of-two multiples of the default table
        assert np.isfinite(x).all() and (np.abs(x) <= 2.0 ** 40).all()


def test_wave_partition_counts():
    x = np.zeros((2, 8, 2))
    x[0, :4] = 2.0 ** 51          # step 0, wave 0: all at the bound
    x[1, 4:8] = -2.0 ** 52        # step 1, wave 1: all above, negative
    x[1, 0, 0] = np.nextafter(2.0 ** 51, 0)  # step 1, wave 0: below
    x[0, 5, 1] = 2.0 ** 53        # step 0, wave 1: mixed
    assert C.wave_partition(x) == (1, 2, 1)


# ----------------------------------------------------------------------------- window_keys against the oracle's delta
@pytest.mark.parametrize("case", ["crowded", "wide"])
def test_window_keys_restate_the_oracles_delta(case):
    """The keys and first-episode deltas that window_keys counts, summed per key in Python ints, are the
    oracle's q_delta entry for entry (contributions to a key may cancel, so the comparison is of sums,
    not of the set of keys)."""
    if case == "crowded":
        inp, out, q_delta = _crowded_first_episode(40, 16, 20)
        alpha = 1e-5
    else:
        inp, _, out, q_delta = _wide_first_episode()
        alpha = inp.alpha
    keys = C.final_keys(out).ravel()
    v = C.first_episode_delta(out, alpha).ravel()
    acc = {}
    for k, d in zip(keys.tolist(), v.tolist()):
        if d != 0:
            acc[k] = acc.get(k, 0) + d
    want = np.zeros((20 ** 4, 4), np.int64)
    for k, d in acc.items():
        assert -2 ** 63 <= d < 2 ** 63
        want.reshape(-1)[k] = d
    assert not want[:, 3].any()  # actions 0..2 only: the pad column of the device's rows stays empty
    assert np.array_equal(want[:, :3], q_delta)
    # and the count of one window over all scenarios is the number of keys its agent-steps touch
    n = C.window_keys(out, 0, inp.S, window=out["reward"].shape[0], alpha=alpha)
    assert n == [len(acc)]


# ----------------------------------------------------------------------------- the oracle's rounding
def _rint_i64(x):
    return np.rint(np.asarray(x, np.float64)).astype(np.int64)


def test_oracle_rounding_is_exact_round_half_even():
    """np.rint(x).astype(int64), the oracle's f64 -> int64 step, against exact rational arithmetic:
    around +-2^51 and +-2^52 (where the f64 spacing passes 1/2 and 1), half-integers below 2^51, and the
    extreme values of the wide builder."""
    vals = []
    for e in (51, 52):
        b = 2.0 ** e
        x = np.nextafter(b, 0)
        for _ in range(6):  # the six doubles either side of the power of two
            vals.append(x)
            x = np.nextafter(x, 0)
        x = b
        for _ in range(6):
            vals.append(x)
            x = np.nextafter(x, np.inf)
    rs = np.random.RandomState(2)
    halves = np.floor(rs.uniform(0, 2.0 ** 51, 200)) + 0.5
    vals += list(halves) + [0.5, 1.5, 2.5, 2.0 ** 51 - 0.5, 2.0 ** 51 - 1.5, 2.0 ** 50 + 0.5]
    vals += list(rs.uniform(2.0 ** 50, 2.0 ** 53, 200)) + [0.0, 0.49999999999999994, 2.0 ** 62]
    inp, _, out, _ = _wide_first_episode()
    x = (inp.alpha * out["reward"].astype(np.float64)) * DELTA_SCALE
    order = np.argsort(np.abs(x).ravel())
    vals += list(x.ravel()[order[-50:]]) + list(x.ravel()[order[:50]])
    near = np.abs(np.abs(x) - 2.0 ** 51).ravel()
    vals += list(x.ravel()[np.argsort(near)[:50]])
    vals = np.asarray(vals, np.float64)
    vals = np.concatenate([vals, -vals])
    got = _rint_i64(vals)
    for v, g in zip(vals.tolist(), got.tolist()):
        assert g == C.rne_exact(v), (v.hex(), g)


def test_rne_exact_rounds_half_to_even():
    assert [C.rne_exact(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.0 ** 51 - 0.5, -(2.0 ** 51 - 1.5))] == \
        [0, 2, 2, 0, -2, -2, 2 ** 51, -(2 ** 51 - 2)]


def test_replay_codes_shape_and_mix():
    codes = C.replay_codes(np.random.RandomState(1), 9, 1, 6, 16)
    assert codes.shape == (9, 2, 6, 16) and codes.dtype == np.uint8
    assert set(np.unique(codes)) == {0, 1, 2, 255}
    assert 0.3 < (codes != 255).mean() < 0.5
