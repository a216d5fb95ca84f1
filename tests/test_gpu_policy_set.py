"""Policy sets on the device (p2pmg_set_policy_set, p2pmg_policy_set_capture, p2pmg_run_policy) against the
unchanged oracle holding each agent's one-hot table (tests/policy_set_ref.py), bit for bit, and against the
context's own greedy episode after a capture.

Shapes: T = 12; S = 5 and S = 37 leave partial waves and partial workgroups at every lane-group width; the
register forms N in {1, 2, 3, 5, 8, 16}, the LDS-tile form N in {9, 12, 33, 64} and, forced, N = 4; R in
{0, 1, 2} and R + 1 = 9.  Random bytes over {0, 1, 2, 255} drive T_in across the whole band, so the bins of every
axis are crossed and a kernel that read the wrong policy, row or byte could not pass."""
import ctypes as C

import numpy as np
import pytest

import policy_set_ref as ref
import summary_ref
from p2pmicrogrid_amd import _lib
from p2pmicrogrid_amd import day_profile as dayprof
from p2pmicrogrid_amd._lib import P2PMGError
from p2pmicrogrid_amd.engine import DeviceCommunityBatch, default_policy_map, unpack_index

pytestmark = pytest.mark.gpu
T = 12
REC = ref.REC


def _run_case(S, N, R, kernel="auto", T=T, **kw):
    inp, pol, th, cap, out = ref.reference(S, N, R, T, **kw)
    eng = ref.device_for(inp, N, R, dims=kw.get("dims"), thermal=th, battery=cap)
    try:
        eng.set_policy_set(pol)  # M == A: the identity map
        eng.run_policy(record=REC, kernel=kernel)
        name = eng.last_kernel()
        rec = eng.get_records(REC)
        ref.assert_records_equal(rec, out, (S, N, R, kernel))
        ref.assert_state_equal(eng, out, (S, N, R, kernel))
    finally:
        eng.close()
    return rec, out, name


# ----------------------------------------------------------------- 1. against the oracle, random policies
REGISTER_CASES = [(5, 1, 0), (37, 1, 1), (5, 2, 1), (37, 2, 1), (37, 2, 2), (37, 3, 0), (5, 3, 2), (37, 5, 1), (5, 8, 1),
                  (37, 8, 0), (5, 16, 1), (5, 16, 2)]
TILE_CASES = [(5, 9, 1), (37, 9, 0), (5, 12, 2), (5, 33, 0), (5, 64, 1)]


@pytest.mark.parametrize("S,N,R", REGISTER_CASES)
def test_register_forms_against_the_oracle(S, N, R):
    rec, out, name = _run_case(S, N, R)
    assert name == f"policy_episode_kernel<{N},R1={R + 1}>"
    assert len(np.unique(rec["action"])) == 3                      # every action taken
    assert len(np.unique(unpack_index(rec["index"])[..., 1])) > 2  # several temperature bins are read


@pytest.mark.parametrize("S,N,R", TILE_CASES)
def test_tile_form_against_the_oracle(S, N, R):
    _, _, name = _run_case(S, N, R)
    assert name == f"policy_episode_kernel<{N},tile{16 if N <= 16 else 32 if N <= 32 else 64},R1={R + 1}>"


def test_tile_form_at_a_register_size_equals_the_register_form():
    a, out, name_a = _run_case(5, 4, 1)
    b, _, name_b = _run_case(5, 4, 1, kernel="tile")
    assert name_a == "policy_episode_kernel<4,R1=2>" and name_b == "policy_episode_kernel<4,tile16,R1=2>"
    for k in REC:
        assert np.array_equal(a[k], b[k]), k


def test_nine_rounds():
    """R + 1 = 9: rounds past the eight a general-kernel code word holds."""
    rec, out, name = _run_case(5, 2, 8)
    assert name == "policy_episode_kernel<2,R1=9>" and rec["action"].shape[1] == 9
    assert len(np.unique(unpack_index(rec["index"])[:, 1:, ..., 3])) > 1  # the later rounds' p2p bins differ


def test_per_agent_thermal_and_heat_pump_levels():
    _run_case(5, 3, 1, thermal=True)
    inp, pol, th, _, out = ref.reference(5, 3, 1, T, thermal=True)
    plain = ref.reference(5, 3, 1, T)  # the same inputs and policies at the default thermal values
    assert th is not None and not np.array_equal(out["t_in"], plain[4]["t_in"])


def test_battery_with_mixed_capacities():
    rec, out, name = _run_case(5, 4, 1, battery=True)
    assert name == "policy_episode_kernel<4,R1=2,battery>"
    cap = ref.reference(5, 4, 1, T, battery=True)[3]
    assert (cap == 0).any() and (cap > 0).any() and not np.all(out["soc_final"] == 0.5)


def test_non_default_table_shape():
    _run_case(5, 2, 1, dims=(6, 5, 7, 4))
    _run_case(5, 12, 1, dims=(6, 5, 7, 4))


def test_one_step_horizon_wraps_onto_itself():
    _run_case(5, 2, 1, T=1)
    _run_case(5, 9, 1, T=1)


# ----------------------------------------------------------------- 2. maps
@pytest.mark.parametrize("M,shuffled", [(10, False), (2, False), (1, False), (3, True)])
def test_maps(M, shuffled):
    """M == A, M == N (the role map), M == 1, and an explicit shuffled map with M = 3, at S = 5, N = 2: the
    device equals the oracle fed the policies through the same map."""
    S, N, R = 5, 2, 1
    inp = ref.inputs(S, N, T)
    pol = ref.random_policies(M, 160000, seed=70 + M)
    if shuffled:
        mp = np.random.RandomState(4).permutation(np.arange(S * N) % M).astype(np.int32)
        assert set(mp) == {0, 1, 2} and not np.array_equal(mp, np.arange(S * N) % M)
    else:
        mp = default_policy_map(M, S, N)
    out = ref.oracle_policy_run(inp, N, R, pol, mp)
    eng = ref.device_for(inp, N, R)
    try:
        eng.set_policy_set(pol, policy_of=mp if shuffled else None)
        got_pol, got_map = eng.policy_set()
        assert np.array_equal(got_pol.reshape(M, -1), pol) and np.array_equal(got_map.reshape(-1), mp)
        eng.run_policy(record=REC)
        ref.assert_records_equal(eng.get_records(REC), out, (M, shuffled))
        ref.assert_state_equal(eng, out, (M, shuffled))
    finally:
        eng.close()


# ----------------------------------------------------------------- 3. capture equals greedy
@pytest.mark.parametrize("shared_q", [False, True, "role"])
@pytest.mark.parametrize("q_dtype", ["f64", "f32"])
def test_capture_then_run_policy_equals_the_greedy_episode(shared_q, q_dtype):
    S, N, R = 6, 2, 1
    inp = ref.inputs(S, N, T)
    eng = ref.device_for(inp, N, R, shared_q=shared_q, q_dtype=q_dtype, alpha=0.3)
    try:
        for e, eps in enumerate((0.8, 0.5)):
            eng.run_episode("train", "philox", episode=e, epsilon=eps)
            if shared_q:
                eng.apply_q_delta()
        eng.set_policy_set(count=eng.n_tables)
        eng.capture_policies()
        t_in, t_m = eng.get_temperatures()
        eng.run_episode("greedy", record=REC, kernel="general")
        assert eng.last_kernel().startswith("episode_kernel<")
        want = eng.get_records(REC)
        want_t, want_r = eng.get_temperatures(), eng.episode_reward().copy()
        eng.set_temperatures(t_in, t_m)
        eng.run_policy(record=REC)
        assert eng.last_kernel().startswith("policy_episode_kernel<")
        got = eng.get_records(REC)
        for k in REC:
            assert np.array_equal(got[k], want[k]), k
        got_t = eng.get_temperatures()
        assert np.array_equal(got_t[0], want_t[0]) and np.array_equal(got_t[1], want_t[1])
        assert np.array_equal(eng.episode_reward(), want_r)
        pol = eng.policy_set()[0]
        assert np.array_equal(pol, eng.greedy_policy())
        assert (pol != 255).any()  # training wrote rows
        # a partial capture: one table into another slot, the rest untouched
        if eng.n_tables > 1:
            eng.capture_policies(first_table=1, count=1, first_slot=0)
            again = eng.policy_set()[0]
            assert np.array_equal(again[0], pol[1]) and np.array_equal(again[1:], pol[1:])
    finally:
        eng.close()


# ----------------------------------------------------------------- 4. independence
def test_the_set_and_the_tables_do_not_touch_each_other():
    S, N, R = 5, 2, 1
    inp = ref.inputs(S, N, T)
    eng = ref.device_for(inp, N, R, shared_q=False, q_dtype="f64", alpha=0.3)
    try:
        pol = ref.random_policies(S * N, 160000, seed=8)
        eng.set_policy_set(pol)
        eng.run_episode("train", "philox", episode=0, epsilon=0.7)
        eng.policy_mark()
        eng.run_episode("train", "philox", episode=1, epsilon=0.7)
        assert np.array_equal(eng.policy_set()[0].reshape(S * N, -1), pol)
        q = eng.get_q()
        changes = eng.policy_changes(remark=False)
        assert q.any() and changes["changed"].sum() + changes["newly_visited"].sum() > 0
        eng.set_temperatures(inp.t_in0, inp.t_m0)
        eng.run_policy(record=REC)
        assert np.array_equal(eng.get_q(), q)
        again = eng.policy_changes(remark=False)
        assert all(np.array_equal(again[k], changes[k]) for k in changes)  # the mark snapshot is as it was
        eng.zero_q()
        assert not eng.get_q().any()
        assert np.array_equal(eng.policy_set()[0].reshape(S * N, -1), pol)
    finally:
        eng.close()


# ----------------------------------------------------------------- 5. downstream
def test_summary_profile_and_last_kernel_after_run_policy():
    S, N, R = 5, 3, 1
    inp, pol, th, _, out = ref.reference(S, N, R, T, thermal=True)
    eng = ref.device_for(inp, N, R, thermal=th)
    try:
        eng.set_policy_set(pol)
        eng.run_policy(record=REC)
        assert eng.last_kernel() == "policy_episode_kernel<3,R1=2>" and eng.last_kernel_ms() > 0
        rec = eng.get_records(REC)
        thm = eng.get_thermal()
        lower, upper = thm[..., 1], thm[..., 2]
        want = summary_ref.summary(rec, eng.get_hp_levels(), inp.load_w, inp.pv_w, lower, upper)
        s = eng.episode_summary()
        assert np.array_equal(np.stack([s["agent"][n] for n in summary_ref.FIELDS], axis=-1), want[0])
        assert np.array_equal(np.stack([s["scenario"][n] for n in summary_ref.FIELDS], axis=-1), want[1])
        groups = np.arange(S) % 2
        got = eng.day_profile(period=4, groups=groups)
        ref_arrays = dayprof.from_records(rec, eng.get_hp_levels(), inp.load_w, inp.pv_w, lower, upper, period=4, groups=groups)
        for g, w in zip(got, ref_arrays):
            assert np.array_equal(g, w)
    finally:
        eng.close()


# ----------------------------------------------------------------- 6. refusals
def _raises(match):
    return pytest.raises(P2PMGError, match=match)


def test_refusals_leave_the_set_intact():
    S, N, R = 5, 2, 1
    inp = ref.inputs(S, N, T)
    eng = ref.device_for(inp, N, R, shared_q="role")
    try:
        with _raises(r"STATE.*set_policy_set first"):
            eng.run_policy()
        with _raises(r"STATE.*set_policy_set first"):
            eng.capture_policies()
        assert eng.policy_set() == (None, None)
        pol = ref.random_policies(3, 160000, seed=9)
        mp = (np.arange(S * N) % 3).astype(np.int32)
        eng.set_policy_set(pol, policy_of=mp)

        def intact():
            p, m = eng.policy_set()
            assert np.array_equal(p.reshape(3, -1), pol) and np.array_equal(m.reshape(-1), mp)
        for byte in (3, 254):
            bad = pol.copy()
            bad[2, 159999] = byte
            with _raises(rf"INVALID.*byte {byte} at policy 2, state 159999"):
                eng.set_policy_set(bad, policy_of=mp)
            intact()
        bad_map = mp.copy()
        bad_map[7] = 3
        with _raises(r"INVALID.*policy_of\[7\] = 3 outside \[0, 3\)"):
            eng.set_policy_set(pol, policy_of=bad_map)
        intact()
        with _raises(r"INVALID.*without policy_of, count must be A, N or 1"):
            eng.set_policy_set(pol)  # M = 3 is neither 10, 2 nor 1
        intact()
        with _raises(r"INVALID.*count must be positive"):
            eng.set_policy_set(count=-1)
        intact()
        # capture ranges: the context holds N = 2 role tables, the set 3 slots
        for args in ((0, 3, 0), (2, 1, 0), (-1, 1, 0), (0, -1, 0)):
            with _raises(r"INVALID.*policy_set_capture: bad table range"):
                eng.capture_policies(*args)
            intact()
        for args in ((0, 2, 2), (0, 1, 3), (0, 1, -1)):
            with _raises(r"INVALID.*policy_set_capture: bad slot range"):
                eng.capture_policies(*args)
            intact()
        eng.capture_policies(0, 0, 3)  # an empty range is no error
        with _raises(r"INVALID.*every P2PMG_REC_\* but LOSS"):
            eng.run_policy(record=("loss",))
        assert eng.L.p2pmg_run_policy_ex(eng._ctx, 0, _lib.FLAG_GENERAL_KERNEL) == 1  # P2PMG_E_INVALID
        intact()
        eng.run_policy(record=("cost",))  # and the set still runs
        eng.set_policy_set(count=0)
        assert eng.policy_set() == (None, None)
        with _raises(r"STATE.*set_policy_set first"):
            eng.run_policy()
    finally:
        eng.close()


def test_refused_on_a_dqn_context_and_on_two_actions():
    from p2pmicrogrid_amd.dqn import DeviceDQNBatch
    d = DeviceDQNBatch(2, 2, 1, T, capacity=32)
    try:
        pol = np.zeros((1, 160000), np.uint8)
        for rc in (d.L.p2pmg_set_policy_set(d._ctx, 1, pol.ctypes.data, None), d.L.p2pmg_run_policy(d._ctx, 0),
                   d.L.p2pmg_policy_set_capture(d._ctx, 0, 0, 0),
                   d.L.p2pmg_get_policy_set(d._ctx, C.byref(C.c_int(0)), None, None)):
            assert rc == 4  # P2PMG_E_STATE
        assert b"DQN context" in d.L.p2pmg_last_error(d._ctx)
    finally:
        d.close()
    two = DeviceCommunityBatch(2, 2, 1, T, n_actions=2, shared_q=True)
    try:
        two.set_policy_set(np.array([[0, 1, 255] * 53333 + [0]], np.uint8))  # a set of its own actions is held
        with _raises(r"INVALID.*byte 2"):
            two.set_policy_set(np.full((1, 160000), 2, np.uint8))
        two.capture_policies()  # and captured (an all-zero table: every row unvisited)
        assert np.all(two.policy_set()[0] == 255)
        with _raises(r"UNSUPPORTED.*3 actions"):
            two.run_policy()
    finally:
        two.close()
