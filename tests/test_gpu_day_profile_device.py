"""p2pmg_day_profile on the device: the four arrays bit for bit (np.array_equal) the NumPy definition
(tests/day_profile_ref.py) applied to the ORACLE's episode, for every kernel family and record layout a launch
can leave (tests/day_profile_cases.py), every argument variant, every path of the pass (LDS tile with several
step slices and several agent tiles per workgroup, the global fallback: P2PMG_DAYPROF_TILE_BYTES), plus the
error states, merging, isolation from the rest of the context, chained launches and the dict form."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import day_profile_cases as cases
import summary_cases
from summary_cases import RECORDS
from test_gpu_summary import _device, _launch

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = ("sums", "extrema", "com_sums", "com_extrema")
# the LDS a workgroup may use: the default; room for a few slots of one group only (several step slices, and
# the fallback for the labelled variants of the 16-agent case); less than one slot of any case (the fallback)
TILES = {"default": None, "slices": "6000", "fallback": "300"}


@pytest.fixture(scope="module")
def launched():
    """name -> an engine whose last launch is the case's, shared by the tests that only read it."""
    held = {}

    def get(name):
        if name not in held:
            e = cases.episode(name)
            eng = _device(e["case"], e["inp"])
            _launch(e["case"], e["inp"], eng)
            held[name] = eng
        return held[name]
    yield get
    for eng in held.values():
        eng.close()


def _assert_equal(got, want, tag):
    assert len(got) == 4
    for g, w, what in zip(got, want, NAMES):
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, what, g.shape, w.shape, g.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            k = tuple(bad[0])
            raise AssertionError(f"{tag} {what}: {len(bad)} of {g.size} differ, first at {k}: {g[k]!r} != {w[k]!r}")


def _tile(monkeypatch, tile):
    if TILES[tile] is None:
        monkeypatch.delenv("P2PMG_DAYPROF_TILE_BYTES", raising=False)
    else:
        monkeypatch.setenv("P2PMG_DAYPROF_TILE_BYTES", TILES[tile])


@pytest.mark.parametrize("name", cases.CASES)
def test_profile_matches_oracle(name, launched, monkeypatch):
    _tile(monkeypatch, "default")
    e = cases.episode(name)
    eng = launched(name)
    assert e["case"].last_kernel in eng.last_kernel(), eng.last_kernel()
    got = eng.day_profile()
    _assert_equal(got, cases.want(name), name)
    assert np.all(got[0][..., 0] == e["case"].S) and np.all(got[2][..., 0] == e["case"].S)
    if e["case"].kind == "rule":
        assert np.all(got[0][..., 2] == 0)


@pytest.mark.parametrize("tile", list(TILES))
@pytest.mark.parametrize("name", cases.VARIANT_CASES)
def test_argument_variants_on_every_path(name, tile, launched, monkeypatch):
    _tile(monkeypatch, tile)
    eng = launched(name)
    vs = cases.variants(cases.episode(name)["case"])
    assert len(vs) >= 12
    for tag, kw in vs:
        _assert_equal(eng.day_profile(**kw), cases.want(name, tag), f"{name} {tag} {tile}")


@pytest.mark.parametrize("tile", list(TILES))
def test_one_group_per_scenario(tile, launched, monkeypatch):
    _tile(monkeypatch, tile)
    e = cases.episode("sq16_many")
    S = e["case"].S
    got = launched("sq16_many").day_profile(groups=np.arange(S))
    assert got[0].shape[0] == S == 70 and np.all(got[0][..., 0] == 1)
    _assert_equal(got, cases.want_from(e, groups=np.arange(S)), "arange")


@pytest.mark.parametrize("name", ["sq16_many", "general"])
def test_equals_the_host_form_on_the_launch_own_records(name, launched, monkeypatch):
    """The device's profile against day_profile.from_records of what get_records returns from the same launch
    (a packed and a plain layout), and through ctypes each output pointer alone."""
    from p2pmicrogrid_amd import _lib, day_profile
    _tile(monkeypatch, "default")
    e = cases.episode(name)
    c, inp = e["case"], e["inp"]
    eng = launched(name)
    assert bool(eng.last_kernel().startswith("episode_sq16_kernel")) == (name == "sq16_many")
    rec = eng.get_records(RECORDS)
    lower, upper = c.bounds()
    mod3 = np.arange(c.S) % 3
    for kw in ({}, {"period": 7, "steps": (2, c.T - 1), "groups": mod3, "n_groups": 3}):
        want = day_profile.from_records(rec, eng.get_hp_levels(), inp.load_w, inp.pv_w, lower, upper, **kw)
        _assert_equal(eng.day_profile(**kw), want, f"{name} {sorted(kw)}")
    G, P = C.c_int32(0), C.c_int32(0)
    args = _lib.DayProfileArgs(0, 0, -1, 0, -1, 0, None)
    assert eng.L.p2pmg_day_profile_shape(eng._ctx, C.byref(args), C.byref(G), C.byref(P)) == _lib.P2PMG_OK
    assert (G.value, P.value) == (1, c.T)
    for k in range(4):
        out = np.zeros_like(cases.want(name)[k])
        ptrs = [None] * 4
        ptrs[k] = out.ctypes.data
        assert eng.L.p2pmg_day_profile(eng._ctx, C.byref(args), *ptrs) == _lib.P2PMG_OK
        assert np.array_equal(out, cases.want(name)[k]), NAMES[k]
    assert eng.L.p2pmg_day_profile(eng._ctx, C.byref(args), None, None, None, None) == 1  # P2PMG_E_INVALID


@pytest.mark.parametrize("name", ["fast_greedy", "general"])
def test_errors_name_what_is_wrong_and_leave_the_context_usable(name):
    from p2pmicrogrid_amd._lib import P2PMGError
    e = cases.episode(name)
    c, inp = e["case"], e["inp"]
    want = cases.want_from(e)
    eng = _device(c, inp)
    with pytest.raises(P2PMGError, match=r"STATE.*day_profile: no episode has run.*cost"):
        eng.day_profile()
    _launch(c, inp, eng, record=("reward", "cost"))  # fast kernel: the narrow rows
    with pytest.raises(P2PMGError, match=r"STATE.*did not record grid, p2p, t_in, action"):
        eng.day_profile()
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    _launch(c, inp, eng, record=("reward", "cost", "grid", "p2p", "t_in"))
    with pytest.raises(P2PMGError, match=r"STATE.*did not record action$"):
        eng.day_profile()
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    _launch(c, inp, eng)
    lab = np.arange(c.S) % 2
    for kw, what in (({"period": c.T + 1}, "period"), ({"scenarios": (0, c.S + 1)}, "scenario range"),
                     ({"steps": (c.T, c.T + 1)}, "step range"), ({"groups": lab, "n_groups": 1}, "label"),
                     ({"groups": lab - 2 * (lab == 0)}, "label")):
        with pytest.raises(P2PMGError, match=rf"INVALID day_profile: .*{what}"):
            eng.day_profile(**kw)
    with pytest.raises(ValueError):
        eng.day_profile(groups=lab[:-1])
    # a valid call afterwards is right, empty ranges included
    _assert_equal(eng.day_profile(), want, name)
    empty = eng.day_profile(steps=(4, 4), period=8)
    _assert_equal(empty, cases.want_from(e, steps=(4, 4), period=8), name + " empty")
    assert not empty[0].any() and np.all(empty[1][..., 0::2] == np.inf) and np.all(empty[3][..., 1] == -np.inf)
    _assert_equal(eng.day_profile(scenarios=(1, 1)), cases.want_from(e, scenarios=(1, 1)), name + " no scenario")
    # without the reward record column 2 is 0, everything else as before
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    _launch(c, inp, eng, record=[r for r in RECORDS if r != "reward"])
    got = eng.day_profile()
    assert want[0][..., 2].any() and not got[0][..., 2].any()
    assert np.array_equal(np.delete(got[0], 2, -1), np.delete(want[0], 2, -1))
    assert all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))
    _assert_equal(got, cases.want_from(e, reward=False), name + " no reward, reference")
    eng.close()


def test_scenario_ranges_merge_to_the_whole(launched, monkeypatch):
    from p2pmicrogrid_amd.distributed import merge_day_profiles
    _tile(monkeypatch, "default")
    eng = launched("sq16_many")
    S = cases.episode("sq16_many")["case"].S
    mod3 = np.arange(S) % 3
    for kw in ({}, {"period": 12, "groups": mod3, "n_groups": 3}):
        whole = eng.day_profile(**kw)
        _assert_equal(whole, cases.want("sq16_many", "whole") if not kw else cases.want_from(cases.episode("sq16_many"), **kw), "whole")
        for k in (3, 8, 64, 69):  # inside a wave; at multiples of 64 / N = 4 scenarios; the last scenario alone
            parts = [eng.day_profile(scenarios=(0, k), **kw), eng.day_profile(scenarios=(k, S), **kw)]
            _assert_equal(merge_day_profiles(parts), whole, f"k = {k}")
            _assert_equal(merge_day_profiles(parts[::-1]), whole, f"k = {k}, reversed")


def test_two_engines_merge_to_the_two_scenario_engine(launched, monkeypatch):
    from p2pmicrogrid_amd.distributed import merge_day_profiles
    _tile(monkeypatch, "default")
    e = cases.episode("general")
    c, inp = e["case"], e["inp"]
    parts = []
    for s in range(c.S):
        one = dataclasses.replace(c, S=1)
        inp1 = summary_cases.Inputs(inp.time, *(getattr(inp, k)[s:s + 1] for k in ("t_out", "load_w", "pv_w", "max_in", "t_in0", "t_m0")))
        eng = _device(one, inp1)
        eng.set_q(c.tables()[s * c.N:(s + 1) * c.N])
        _launch(one, inp1, eng)
        parts.append(eng.day_profile(period=12))
        assert np.all(parts[-1][0][..., 0] == c.T // 12)
        eng.close()
    _assert_equal(merge_day_profiles(parts), launched("general").day_profile(period=12), "two engines")
    _assert_equal(merge_day_profiles(parts), cases.want("general", "period_12"), "two engines, reference")


def test_repeated_calls_and_the_rest_of_the_context(launched, monkeypatch):
    _tile(monkeypatch, "default")
    eng = launched("sq16_many")
    S = cases.episode("sq16_many")["case"].S
    summary = eng.episode_summary()
    rec = eng.get_records(RECORDS)
    a = eng.day_profile()
    b = eng.day_profile()
    _assert_equal(b, a, "twice")
    eng.day_profile(period=7, groups=np.arange(S) % 3, scenarios=(3, S - 3))  # larger G, other rows, labels uploaded
    eng.day_profile(steps=(0, 0))
    _assert_equal(eng.day_profile(), a, "after other arguments")
    _assert_equal(eng.day_profile(period=7), cases.want("sq16_many", "period_7"), "no labels left behind")
    after = eng.episode_summary()
    assert all(np.array_equal(after[p][k], summary[p][k]) for p in summary for k in summary[p])
    assert all(np.array_equal(v, rec[k]) for k, v in eng.get_records(RECORDS).items())


def test_a_profile_between_training_launches_changes_nothing():
    e = cases.episode("fast_train")
    c, inp = e["case"], e["inp"]
    ends = []
    for profile in (True, False):
        eng = _device(c, inp)
        _launch(c, inp, eng)
        if profile:
            _assert_equal(eng.day_profile(), cases.want("fast_train"), "between")
            eng.day_profile(period=7, groups=np.arange(c.S) % 2)
        eng.run_episode("train", "philox", episode=c.episode + 1, epsilon=c.eps, record=RECORDS, kernel=c.kernel)
        ends.append((eng.get_q(), eng.get_temperatures(), eng.get_records(RECORDS), eng.day_profile()))
        eng.close()
    (qa, ta, ra, pa), (qb, tb, rb, pb) = ends
    assert np.array_equal(qa, qb) and all(np.array_equal(x, y) for x, y in zip(ta, tb))
    assert all(np.array_equal(ra[k], rb[k]) for k in ra)
    _assert_equal(pa, pb, "after the second launch")
    assert not np.array_equal(pa[0], cases.want("fast_train")[0])


def test_after_a_chain_the_profile_is_the_last_episodes():
    """run_episodes of 3 chained episodes with full records == the third episode launched alone."""
    from p2pmicrogrid_amd import day_profile
    c = summary_cases.CASES["fast_train"]
    inp = c.inputs()
    eps = [0.8, 0.7, 0.6]
    a = _device(c, inp)
    a.run_episodes(0, eps, reset_sigma=0.3, record=RECORDS)
    assert a.last_kernel().startswith("episode_fast_kernel")
    b = _device(c, inp)
    b.run_episodes(0, eps[:2], reset_sigma=0.3, next_epsilons=eps[2:])
    b.run_episode("train", "philox", episode=2, epsilon=eps[2], record=RECORDS, reset_sigma=0.3)
    got = a.day_profile(period=8)
    _assert_equal(got, b.day_profile(period=8), "chain")
    lower, upper = c.bounds()
    _assert_equal(got, day_profile.from_records(a.get_records(RECORDS), a.get_hp_levels(), inp.load_w, inp.pv_w, lower, upper,
                                                period=8), "chain records")
    assert not np.array_equal(got[0], cases.want_from(cases.episode("fast_train"), period=8)[0])  # not episode 3's of the case
    a.close()
    b.close()


def test_dict_form_and_kwh(launched, monkeypatch):
    from p2pmicrogrid_amd import day_profile
    _tile(monkeypatch, "default")
    eng = launched("general")
    arrays = eng.day_profile(period=12)
    for kwh, scale in ((False, 1.0), (True, 15.0 / 60.0 * 1e-3)):
        got = eng.day_profile(period=12, as_dict=True, kwh=kwh)
        want = day_profile.as_dict(*arrays, energy_scale=scale)
        assert list(got) == ["agent", "community"]
        for part in want:
            assert list(got[part]) == list(want[part])
            assert all(np.array_equal(got[part][k], want[part][k], equal_nan=True) for k in want[part]), (part, kwh)
    assert got["agent"]["load"].shape == (1, 12, 5) and got["community"]["net_grid"].shape == (1, 12)
