"""Day profiles without a GPU: p2pmicrogrid_amd.day_profile (from_records, merge, as_dict) against the
reference helper (tests/day_profile_ref.py) on the oracle's episodes, the helper against a loop that forms every
term with Python scalars, the fixed-point identities, the bookkeeping of groups, ranges and periods, and the
non-triviality of the expected arrays on every input set."""
import numpy as np
import pytest

import day_profile_cases as cases
import day_profile_ref as ref

F32, I64 = np.float32, np.int64


def _equal(got, want):
    return all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want) == 4


@pytest.mark.parametrize("name,kw", [
    ("fast_train", {}), ("fast_train", {"period": 7, "steps": (3, 90)}),
    ("fast_train", {"groups": [2, 0, -1], "n_groups": 4, "period": 12, "scenarios": (0, 3)}),
    ("mixed", {"period": 12}),     # per-agent heat pumps and comfort bands
    ("rule", {"period": 0}),       # no reward record, actions 0 and 2 only; period 0 is T
    ("battery", {"groups": [1, 1, 0], "n_groups": 2, "scenarios": (1, 3)}),
    ("one_step", {}), ("one_agent", {"period": 96})])
def test_helper_equals_the_python_scalar_loop(name, kw):
    """``profile`` (vectorised) against ``profile_loops``, which forms every term itself from the records."""
    e = cases.episode(name)
    args = (e["out"], e["levels"], e["inp"].load_w, e["inp"].pv_w, e["lower"], e["upper"])
    assert _equal(ref.profile(*args, reward=e["reward"], **kw), ref.profile_loops(*args, reward=e["reward"], **kw))


def _package(e, reward=None, **kw):
    """day_profile.from_records on the episode's records (without the reward record where it was not kept)."""
    from p2pmicrogrid_amd import day_profile
    rec = {k: e["out"][k] for k in day_profile.RECORDS}
    if e["reward"] if reward is None else reward:
        rec["reward"] = e["out"]["reward"]
    return day_profile.from_records(rec, e["levels"], e["inp"].load_w, e["inp"].pv_w, e["lower"], e["upper"], **kw)


@pytest.mark.parametrize("name", cases.CASES)
def test_from_records_matches_the_reference(name):
    e = cases.episode(name)
    assert _equal(_package(e), cases.want(name))
    tag = "period_7" if e["case"].T >= 7 else "period_1"
    assert _equal(_package(e, **dict(cases.variants(e["case"]))[tag]), cases.want(name, tag)), tag
    if e["reward"]:  # without the reward record column 2 is 0 and nothing else moves
        assert _equal(_package(e, reward=False), cases.want_from(e, reward=False))


@pytest.mark.parametrize("name", cases.VARIANT_CASES)
def test_from_records_periods_ranges_and_groups(name):
    e = cases.episode(name)
    for tag, kw in cases.variants(e["case"]):
        assert _equal(_package(e, **kw), cases.want(name, tag)), tag


def test_from_records_against_the_scalar_loop_and_its_errors():
    from p2pmicrogrid_amd import day_profile
    e = cases.episode("mixed")
    kw = {"groups": [1, -1, 0, 1], "n_groups": 3, "period": 7, "steps": (3, 90)}
    args = (e["out"], e["levels"], e["inp"].load_w, e["inp"].pv_w, e["lower"], e["upper"])
    assert _equal(_package(e, **kw), ref.profile_loops(*args, **kw))
    assert _equal(_package(e, period=0, n_groups=0), cases.want("mixed"))
    for bad in ({"period": 97}, {"period": -1}, {"steps": (5, 97)}, {"scenarios": (2, 5)}, {"scenarios": (2, 1)},
                {"groups": [0, 1, 2, 0], "n_groups": 2}, {"groups": [0, -2, 0, 0]}, {"groups": [0, 0]}):
        with pytest.raises(ValueError):
            _package(e, **bad)
    with pytest.raises(ValueError, match="lack grid, action"):
        day_profile.from_records({k: e["out"][k] for k in ("cost", "p2p", "t_in")}, *args[1:])


def test_argument_conventions():
    e = cases.episode("fast_train")
    whole = cases.want_from(e)
    assert _equal(cases.want_from(e, period=0), whole) and _equal(cases.want_from(e, period=96, n_groups=0), whole)
    assert _equal(cases.want_from(e, steps=(0, 96), scenarios=(0, 3), groups=[0, 0, 0]), whole)
    empty = cases.want_from(e, steps=(96, 96))  # an empty range: every row empty
    assert not empty[0].any() and np.all(empty[1][..., 0::2] == np.inf) and np.all(empty[3][..., 1] == -np.inf)
    for bad in ({"period": 97}, {"period": -1}, {"steps": (5, 97)}, {"steps": (-1, 4)}, {"scenarios": (2, 4)},
                {"scenarios": (2, 1)}, {"groups": [0, 1, 2], "n_groups": 2}, {"groups": [0, -2, 0]}, {"groups": [0, 0]}):
        with pytest.raises(ValueError):
            cases.want_from(e, **bad)


def test_import_minus_export_is_fix_of_the_net_for_every_sample():
    e = cases.episode("sq16_many")
    terms, values, G_t = ref.sample_terms(e["out"], e["levels"], e["inp"].load_w, e["inp"].pv_w, e["lower"], e["upper"])
    assert np.array_equal(terms[..., 3] - terms[..., 4], ref.fix(values[..., 1], ref.SHIFT_W))
    assert np.array_equal(terms[..., 5] - terms[..., 6], ref.fix(values[..., 2], ref.SHIFT_W))
    assert np.array_equal(ref.fix(np.where(G_t > 0, G_t, 0), 16) - ref.fix(np.where(G_t < 0, -G_t, 0), 16), ref.fix(G_t, 16))
    # fix rounds to nearest even and is odd
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.0 + 2.0 ** -20], F32)
    assert ref.fix(x, 0).tolist() == [0, 2, 2, 0, -2, 3] and np.array_equal(ref.fix(-x, 16), -ref.fix(x, 16))


@pytest.mark.parametrize("name", ["fast_train", "sq16_many", "general", "rule"])
def test_which_values_convert_exactly(name):
    """An f32 x converts exactly at scale 2^-k iff it is a multiple of 2^-k, which every x with
    |x| >= 2^(23 - k) is (its ulp is at least 2^-k): 128 W, 0.5 degC and 2^-5 = 0.03125 money.  Below that
    the error is at most half a step, 2^-(k + 1).  Indoor temperatures always lie above their threshold and
    most powers do; a step's cost and reward are often below 0.03, so the money columns are the inexact ones.
    Shares of exact values on the oracle's records (fast_train, sq16_many, general, rule): T_in 1.00 on
    all; grid above 0.97; cost 0.60, 0.69, 0.73, 0.76; reward 0.75 to 0.97.  The means of the money columns
    are therefore exact to 2^-29 per sample, not bit-exact images of the f32 values."""
    e = cases.episode(name)
    _, values, _ = ref.sample_terms(e["out"], e["levels"], e["inp"].load_w, e["inp"].pv_w, e["lower"], e["upper"],
                                    e["reward"])
    cols = [(values[..., 0], 24), (values[..., 1], 16), (values[..., 2], 16), (values[..., 3], 28)]
    if e["reward"]:
        cols.append((np.asarray(e["out"]["reward"], F32), 28))
    for v, k in cols:
        back = ref.fix(v, k).astype(np.float64) * 2.0 ** -k
        big = np.abs(v) >= 2.0 ** (23 - k)
        assert np.array_equal(back[big], v[big].astype(np.float64)), k
        assert np.all(np.abs(back - v.astype(np.float64)) <= 2.0 ** -(k + 1)), k
    t_in, cost = values[..., 0], values[..., 3]
    assert np.all(np.abs(t_in) >= 0.5)  # indoor temperatures: every one is exact
    assert (ref.fix(cost, 28).astype(np.float64) * 2.0 ** -28 != cost).any()  # some cost is not


def test_group_range_and_period_bookkeeping():
    e = cases.episode("general")  # 2 x 5 agents, 96 steps
    c = e["case"]
    whole = cases.want_from(e)
    assert whole[0].shape == (1, 96, 5, 16) and whole[1].shape == (1, 96, 5, 8)
    assert whole[2].shape == (1, 96, 4) and whole[3].shape == (1, 96, 2)
    assert np.all(whole[0][..., 0] == c.S) and np.all(whole[2][..., 0] == c.S)
    # period 7 over 96 steps: slots 0..4 hold 14 steps, 5 and 6 hold 13
    p7 = cases.want_from(e, period=7)
    assert p7[0][0, :, 0, 0].tolist() == [14 * c.S] * 5 + [13 * c.S] * 2
    assert np.array_equal(p7[0].sum(axis=1), whole[0].sum(axis=1))
    assert np.array_equal(p7[1][..., 0::2].min(axis=1), whole[1][..., 0::2].min(axis=1))
    # folding everything into one slot, and a step range
    p1 = cases.want_from(e, period=1, steps=(10, 20))
    assert p1[0].shape == (1, 1, 5, 16) and np.array_equal(p1[0][0, 0], whole[0][0, 10:20].sum(axis=0))
    # a group with no scenario, and a left-out scenario: group 0 holds scenario 1 alone, 1 and 2 stay empty
    g = cases.want_from(e, groups=[-1, 0], n_groups=3)
    only1 = cases.want_from(e, scenarios=(1, 2))
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(g, only1))
    assert np.all(g[0][1:] == 0) and np.all(g[2][1:] == 0)
    assert np.all(g[1][1:, ..., 0::2] == np.inf) and np.all(g[1][1:, ..., 1::2] == -np.inf)
    assert np.all(g[3][1:, :, 0] == np.inf) and np.all(g[3][1:, :, 1] == -np.inf)
    # the groups partition the scenarios: they add up to the whole
    two = cases.want_from(e, groups=[1, 0], n_groups=2)
    assert np.array_equal(two[0].sum(axis=0), whole[0][0]) and np.array_equal(two[2].sum(axis=0), whole[2][0])


def test_merge_of_two_halves_is_the_whole():
    from p2pmicrogrid_amd.distributed import merge_day_profiles
    e = cases.episode("sq16_many")
    kw = {"groups": np.arange(70) % 3, "n_groups": 3, "period": 7}
    whole = cases.want_from(e, **kw)
    parts = [_package(e, scenarios=r, **kw) for r in ((0, 33), (33, 70))]
    assert _equal(merge_day_profiles(parts), whole)
    assert _equal(merge_day_profiles(parts[::-1]), whole)
    assert not np.array_equal(parts[0][0], whole[0])
    with pytest.raises(ValueError):
        merge_day_profiles([])


def test_profile_dict_means_and_shares():
    from p2pmicrogrid_amd.day_profile import as_dict as profile_dict
    e = cases.episode("fast_train")
    raw = cases.want_from(e, groups=[0, 0, 2], n_groups=3, period=12)
    d = profile_dict(*raw)
    ag, com = d["agent"], d["community"]
    assert ag["cost"].shape == (3, 12, 2) and com["net_grid"].shape == (3, 12)
    assert np.all(np.isnan(ag["cost"][1])) and np.all(ag["samples"][1] == 0) and np.all(np.isnan(com["net_grid"][1]))
    n = raw[0][..., 0]
    assert np.array_equal(ag["t_in"][0], raw[0][0, ..., 10] * 2.0 ** -24 / n[0])
    assert np.array_equal(ag["net_grid"][2], (raw[0][2, ..., 3] - raw[0][2, ..., 4]) * 2.0 ** -16 / n[2])
    assert np.allclose(ag["action0"][0] + ag["action1"][0] + ag["action2"][0], 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(ag["grid_max"], raw[1][..., 3].astype(np.float64))
    k = profile_dict(*raw, energy_scale=0.25e-3)
    assert np.array_equal(k["agent"]["load"][0], raw[0][0, ..., 8] * (2.0 ** -16 * 0.25e-3) / n[0])
    assert np.array_equal(k["agent"]["cost"][0], ag["cost"][0]) and np.array_equal(k["agent"]["grid_max"], ag["grid_max"])


def test_field_names_scales_and_the_overflow_bound():
    from p2pmicrogrid_amd import day_profile as engine
    assert engine.SUM_FIELDS == ref.SUM_FIELDS and engine.EXTREMA_FIELDS == ref.EXTREMA_FIELDS
    assert engine.COM_SUM_FIELDS == ref.COM_SUM_FIELDS and engine.COM_EXTREMA_FIELDS == ref.COM_EXTREMA_FIELDS
    assert (engine.SHIFT_W, engine.SHIFT_DEG, engine.SHIFT_MONEY) == (ref.SHIFT_W, ref.SHIFT_DEG, ref.SHIFT_MONEY)
    assert len(engine.SUM_SHIFTS) == len(engine.SUM_FIELDS) == 16
    # the shift of each column is the one the definition uses for it: a lone sample of value 1.0 in that column
    one = {k: np.ones((1, 1, 1), F32) for k in ("cost", "reward", "grid", "p2p", "t_in")}
    one["action"] = np.ones((1, 1, 1, 1), np.int64)
    sums = ref.profile(one, np.ones((1, 1, 3), F32), np.ones((1, 1, 1), F32), np.ones((1, 1, 1), F32), F32(3), F32(4))[0][0, 0, 0]
    for name, k, got in zip(engine.SUM_FIELDS, engine.SUM_SHIFTS, sums.tolist()):
        if name in ("grid_export", "p2p_export", "action2"):
            assert got == 0, name
        elif name == "discomfort_deg":
            assert got == 2 << k, name  # 3.0 - 1.0 below the band
        else:
            assert got == 1 << k, (name, k)
    # the most samples a row may hold, at the largest magnitude its scale allows, stay below 2^63 ...
    assert set(engine.SUM_SHIFTS) - {0} == set(engine.MAGNITUDE_BITS)
    for k, bits in engine.MAGNITUDE_BITS.items():
        assert engine.MAX_SAMPLES * 2 ** (k + bits) <= 2 ** 63, k
    # ... and the records of every case lie inside those magnitudes
    for name in cases.CASES:
        e = cases.episode(name)
        terms, _, _ = ref.sample_terms(e["out"], e["levels"], e["inp"].load_w, e["inp"].pv_w, e["lower"], e["upper"], e["reward"])
        for f, k in enumerate(engine.SUM_SHIFTS):
            if k:
                assert np.abs(terms[..., f]).max() < 2 ** (k + engine.MAGNITUDE_BITS[k]), (name, f)


@pytest.mark.parametrize("name", cases.CASES)
def test_expected_arrays_are_non_trivial(name):
    """No column of the expected arrays is vacuous on any input set."""
    e = cases.episode(name)
    c = e["case"]
    sums, ext, csums, cext = cases.want(name)
    f = {n: sums[..., k] for k, n in enumerate(ref.SUM_FIELDS)}
    assert sums.shape == (1, c.T, c.N, 16) and np.all(f["samples"] == c.S) and np.all(np.isfinite(ext))
    assert (f["grid_import"] > 0).any() and (f["grid_export"] > 0).any() and (f["importing"] > 0).any()
    assert (ext[..., 2] < 0).any() and (ext[..., 3] > 0).any()
    if c.N >= 2:  # one agent has no peers: its p2p power is 0 by construction
        assert (f["p2p_import"] > 0).any() and (f["p2p_export"] > 0).any()
        assert (ext[..., 4] < 0).any() and (ext[..., 5] > 0).any()
    assert (f["discomfort_steps"] > 0).any() and (f["discomfort_deg"] > 0).any()
    assert (f["cost"] != 0).any() and (f["load"] > 0).any() and (f["pv"] > 0).any() and (f["t_in"] > 0).any()
    if c.kind == "rule":  # off or at full power, and no reward
        assert np.all(f["reward"] == 0) and np.all(f["action1"] == 0) and (f["action2"] > 0).any()
        assert (f["action2"] < f["samples"]).any()
    else:
        assert (f["reward"] != 0).any()
    if c.kind == "tabular" and c.T > 1:  # every action is taken somewhere
        assert (f["action1"] > 0).any() and (f["action2"] > 0).any() and (f["samples"] - f["action1"] - f["action2"] > 0).any()
    if c.T > 1 and not (c.pumps and 0.0 in c.pumps):
        assert (f["hp"] > 0).any()
    # the community's net load has both signs somewhere unless the case is a single step
    assert (csums[..., 1] > 0).any() or (csums[..., 2] > 0).any()
    assert np.all(csums[..., 0] == c.S) and np.all(cext[..., 0] <= cext[..., 1])
    if c.S > 1:
        assert (ext[..., 0] < ext[..., 1]).any()  # the extrema are not the mean


@pytest.mark.parametrize("name", cases.VARIANT_CASES)
def test_variants_differ_from_the_whole(name):
    e = cases.episode(name)
    whole = cases.want(name)
    for tag, kw in cases.variants(e["case"]):
        got = cases.want(name, tag)
        G = kw.get("n_groups", 1)
        P = kw.get("period", e["case"].T)
        assert got[0].shape == (G, P, e["case"].N, 16), tag
        assert got[0][..., 0].sum() > 0, tag
        if tag not in ("whole", "period_96"):  # period = T = 96 is the whole, spelt out
            assert got[0].shape != whole[0].shape or not np.array_equal(got[0], whole[0]), tag
