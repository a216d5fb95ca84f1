"""The shared-table TD-delta path on the device against the oracle, where scenario_batch inputs never
take it (builders and predicates: shared_delta_cases.py; their own checks: test_cpu_shared_delta.py):

  A. more distinct (state, action) keys per 8-step window than the workgroup's LDS hash has slots,
     so that lds_add_by_key's give-up branch (16 probes, then straight to the global replica) runs;
  B. TD deltas on both sides of 2^51, where episode_sq16_kernel's two-instruction f64 -> int64
     rounding hands over to the library conversion, wave by wave;
  C. episode_sq16_kernel at horizons of 1, 2, 3, 7 and 9 steps (its wrapped step indices, and the
     Philox block it shares between an even step and the next odd one), and with uploaded replay codes.

Every comparison is np.array_equal against oracle.restatement.OracleBatch, and every launch's kernel
name is asserted, so that no case can pass on another kernel than the one it names."""
import numpy as np
import pytest

import shared_delta_cases as C
from oracle import philox

pytestmark = pytest.mark.gpu
REC = C.REC
NARROW = ("reward", "cost")


def _cmp(out, rec, tag):
    from p2pmicrogrid_amd.engine import unpack_index
    for k in ("reward", "cost", "grid", "p2p", "t_in"):
        assert np.array_equal(rec[k], out[k]), (tag, k)
    assert np.array_equal(rec["action"], out["action"].astype(np.uint8)), tag
    assert np.array_equal(unpack_index(rec["index"]), out["idx"]), tag


def _episode(eng, ob, tag, kernel_name, mode="train", rng="philox", episode=0, eps=0.5, record=REC, codes=None,
             battery=True, reset_sigma=None, gids=None, **launch):
    """One episode on both sides and everything it leaves behind: records, the int64 delta and the
    table after applying it, the SoC, the episode reward and the temperatures."""
    if codes is not None:
        eng.set_replay_codes(codes)
    eng.run_episode(mode, rng, episode=episode, epsilon=eps, record=record, reset_sigma=reset_sigma, **launch)
    name = eng.last_kernel()
    assert name.startswith(kernel_name) and ",shared" in name, (tag, name)
    if name.startswith("episode_sq16_kernel<"):  # the name says when the launch read pre-pass code words
        want_prepass = mode == "train" and rng == "philox" and launch.get("philox") == "prepass"
        assert (",philox-prepass" in name) == want_prepass, (tag, name)
    out = ob.run_episode(mode, codes=codes, rng=rng, episode=episode, eps=eps, agent_ids=gids)
    if reset_sigma is not None:  # agent.reset() after the episode (community.py:181), as the launch fuses it
        ids = np.arange(ob.S * ob.N) if gids is None else np.asarray(gids).ravel()
        a, b = philox.t0_draws(42, episode + 1, ids, setpoint=21.0, sigma=reset_sigma)
        ob.t_in, ob.t_m = a.reshape(ob.S, ob.N), b.reshape(ob.S, ob.N)
    got = eng.get_records(record)
    if tuple(record) == NARROW:
        assert np.array_equal(got["reward"], out["reward"]) and np.array_equal(got["cost"], out["cost"]), tag
    else:
        _cmp(out, got, tag)
    assert np.array_equal(eng.episode_reward(), out["episode_reward"]), tag
    if battery:
        assert np.array_equal(eng.get_soc(), ob.soc), tag
    t_in, t_m = eng.get_temperatures()
    assert np.array_equal(t_in, ob.t_in) and np.array_equal(t_m, ob.t_m), tag
    if mode == "train":
        delta = eng.get_q_delta().reshape(-1, 3)
        diff = np.nonzero(delta != ob.q_delta)
        assert np.array_equal(delta, ob.q_delta), (tag, "delta", diff[0].size, delta[diff][:4], ob.q_delta[diff][:4])
        eng.apply_q_delta()
        ob.apply_q_delta()
        assert not eng.get_q_delta().any(), tag
    dt = np.float64 if ob.q_dtype == "f64" else np.float32
    assert np.array_equal(eng.get_q(dtype=dt).reshape(ob.q.shape), ob.q), (tag, "table")
    return out


# ----------------------------------------------------------------------------- A. crowded hash
def test_sq16_overfilled_hash_matches_oracle():
    """One launch with a workgroup whose hash overflows and one whose hash does not: S = 40 is a full
    sq16 workgroup (scenarios 0-31, 512 agents) and one of 8 scenarios; T = 20 is windows of 8, 8 and 4
    steps, the last one flushed by t + 1 == T.  In episode 0 (epsilon = 1, zero table) the oracle counts
    3522, 3542 and 1786 distinct keys with a non-zero delta in the windows of scenarios 0-31, and 919,
    905 and 449 in those of scenarios 32-39.  More than 2048 keys cannot sit in 2048 slots, so
    whatever the insertion order, lds_add_by_key's give-up branch ran in the first workgroup.  Then
    two more training episodes (0.6, 0.3) on the table these deltas made, and a greedy one."""
    inp = C.crowded_inputs(40, 16, 20, seed=5)
    pre = C.oracle_for(inp, 1).run_episode("train", rng="philox", episode=0, eps=1.0)
    full, part = C.workgroup_window_keys(pre, C.SQ16_WG_SCENARIOS)
    assert max(full) >= 2300 and max(part) < C.HASH_SLOTS, (full, part)  # the inputs' property, before any launch
    eng, ob = C.engine_for(inp, 1), C.oracle_for(inp, 1)
    for e, eps in enumerate((1.0, 0.6, 0.3)):
        _episode(eng, ob, ("crowded", e), "episode_sq16_kernel<16,f32,R1=2,train", episode=e, eps=eps)
    _episode(eng, ob, "greedy", "episode_sq16_kernel<16,f32,R1=2,greedy", mode="greedy")
    eng.close()


def test_sq16_overfilled_hash_every_replica_and_shards():
    """The same inputs at S = 288, T = 12: nine workgroups, each with more than 3000 distinct keys in
    its first window, so that every one of the 8 delta replicas is written and replica 0 by two
    workgroups.  The folded delta equals the oracle's, and so does the host-side sum of the deltas of
    two contexts that each run a shard of the batch (scenarios 0-159 and 160-287, five and four
    workgroups, Philox counters by global agent id)."""
    S, N, R, T = 288, 16, 1, 12
    inp = C.crowded_inputs(S, N, T, seed=5)
    ob = C.oracle_for(inp, R)
    out = ob.run_episode("train", rng="philox", episode=0, eps=1.0)
    counts = C.workgroup_window_keys(out, C.SQ16_WG_SCENARIOS)
    assert len(counts) == 9 and min(c[0] for c in counts) > C.HASH_SLOTS, counts
    eng = C.engine_for(inp, R)
    eng.run_episode("train", "philox", episode=0, epsilon=1.0, record=REC)
    assert eng.last_kernel().startswith("episode_sq16_kernel<16,f32,R1=2,train"), eng.last_kernel()
    _cmp(out, eng.get_records(REC), "replicas")
    assert np.array_equal(eng.get_q_delta().reshape(-1, 3), ob.q_delta)
    assert np.array_equal(eng.get_soc(), ob.soc)
    eng.close()
    total = np.zeros_like(ob.q_delta)
    for lo, hi in ((0, 160), (160, S)):
        sh = C.engine_for(inp.rows(lo, hi), R, scenario_offset=lo)
        sh.run_episode("train", "philox", episode=0, epsilon=1.0, record=NARROW)
        assert sh.last_kernel().startswith("episode_sq16_kernel<16,f32,R1=2,train"), sh.last_kernel()
        assert np.array_equal(sh.get_record("reward"), out["reward"][:, lo:hi]), (lo, hi)
        total += sh.get_q_delta().reshape(-1, 3)
        sh.close()
    assert np.array_equal(total, ob.q_delta)


# (N, S, scenarios per workgroup, kernel, shared_q, kernel name): S = two workgroups + 3 scenarios
GENERAL_FORMS = [
    (16, 35, 16, "general", True, "episode_kernel<16,f32"),
    (12, 35, 16, "auto", True, "episode_kernel<12,tile16,f32"),
    (2, 259, 128, "auto", True, "episode_kernel<2,f32"),
    (4, 131, 64, "auto", True, "episode_kernel<4,f32"),
    (3, 131, 64, "auto", "role", "episode_kernel<3,f32"),
]


@pytest.mark.parametrize("N,S,spw,kernel,shared,name", GENERAL_FORMS)
def test_general_kernel_crowded_hash_matches_oracle(N, S, spw, kernel, shared, name):
    """episode_kernel's shared-table forms on the crowded builder, T = 20.  Their workgroups hold 256
    lanes, so a window has at most 2048 agent-steps: the hash cannot be overfilled, and no
    order-independent guarantee that the give-up branch ran exists here (the function is the one the
    sq16 case proves).  What these cases add is a table at 66-89 % load, long probe runs and the wrap of
    h + 1 past slot 2047: the oracle counts, in the fullest window of a workgroup, 1797 keys at N = 16,
    1362 at N = 12 (of 1536 agent-steps), 1809 at N = 2, 1820 at N = 4 and 1385 at N = 3 with per-role
    tables, against the ~600 that DESIGN.md describes for the benched inputs.  Per-role tables: the
    oracle has no such form, so role i's delta is rebuilt from the launch's records, as in
    test_gpu_learning.py."""
    R, T = 1, 20
    role = shared == "role"
    inp = C.crowded_inputs(S, N, T, seed=5)
    pre = C.oracle_for(inp, R).run_episode("train", rng="philox", episode=0, eps=1.0)
    counts = C.workgroup_window_keys(pre, spw, role_keys=role)
    assert len(counts) == 3 and max(max(c) for c in counts[:2]) > 1200, counts
    eng = C.engine_for(inp, R, shared_q=shared)
    if role:
        _role_case(eng, inp, N, R, T, name)
        return
    ob = C.oracle_for(inp, R)
    for e, eps in enumerate((1.0, 0.6, 0.3)):
        _episode(eng, ob, ("general", N, e), name, episode=e, eps=eps, kernel=kernel)
    _episode(eng, ob, ("general", N, "greedy"), name, mode="greedy", kernel=kernel)
    eng.close()


def _role_case(eng, inp, N, R, T, name):
    """Per-role tables: with zero tables every agent's trajectory is the shared-table oracle's (all
    rows zero either way), and role i's delta sums agent (s, i)'s updates alone."""
    from p2pmicrogrid_amd.engine import unpack_index
    ob = C.oracle_for(inp, R)
    eng.run_episode("train", "philox", episode=0, epsilon=1.0, record=REC)
    assert eng.last_kernel().startswith(name) and ",roles" in eng.last_kernel(), eng.last_kernel()
    out = ob.run_episode("train", rng="philox", episode=0, eps=1.0)
    rec = eng.get_records(REC)
    _cmp(out, rec, "role")
    assert np.array_equal(eng.get_soc(), ob.soc)
    idx = unpack_index(rec["index"])[:, R]  # [T, S, N, 4]
    srow = ((idx[..., 0] * 20 + idx[..., 1]) * 20 + idx[..., 2]) * 20 + idx[..., 3]
    act = rec["action"][:, R].astype(np.int64)
    v = np.rint((1e-5 * ((rec["reward"].astype(np.float64) + 0.9 * 0.0) - 0.0)) * 2.0 ** 40).astype(np.int64)
    want = np.zeros((N, 20 ** 4, 3), np.int64)
    for i in range(N):
        np.add.at(want[i], (srow[..., i].ravel(), act[..., i].ravel()), v[..., i].ravel())
    assert np.array_equal(eng.get_q_delta().reshape(N, -1, 3), want)
    assert np.array_equal(want.sum(axis=0), ob.q_delta)  # the roles' deltas add up to the one-table delta
    eng.close()


# ----------------------------------------------------------------------------- B. wide deltas
@pytest.mark.parametrize("q_dtype,kernel", [("f32", "auto"), ("f64", "auto"), ("f32", "general"), ("f64", "general")])
def test_wide_deltas_match_oracle(q_dtype, kernel):
    """TD deltas from 2^27 to 2^56 in one batch (wide_delta_inputs; S = 24 is six full sq16 waves).  From
    the oracle's episode-0 rewards (zero table: delta = rint(alpha r 2^40)), over the 72 (step, wave)
    pairs: 64 lie wholly below 2^51 (rne_ll's two-instruction branch), 1 wholly at or above it, 7 have
    lanes on both sides (both the library branch, chosen wave-uniformly).  92 values are negative with a
    magnitude in [2^50, 2^51); 9 of them sit in a wave that lies wholly below 2^51 (wave 5 at step 0,
    largest magnitude 2^50.29), so they go through the two-instruction branch, which is what the
    precondition counts.  The batch's sum of |delta| is 2^61.73 < 2^62, so that no int64 accumulator can
    wrap.  Three episodes: the later ones read table values of 1e5 back, through the f32 cast of
    apply_q_delta where the table is f32.  Every cost operand stays inside [2^-40, 2^40], so that the
    kernels' range-free division keeps to its fast form."""
    inp = C.wide_delta_inputs()
    pre = C.oracle_for(inp, 1, q_dtype, battery=False).run_episode("train", rng="philox", episode=0, eps=0.6)
    x = inp.alpha * pre["reward"].astype(np.float64) * 2.0 ** 40
    below, above, mixed = C.wave_partition(x)
    assert below >= 1 and above >= 1 and mixed >= 1, (below, above, mixed)
    assert C.fast_branch_negative_near_bound(x) >= 1  # x < 0, |x| in [2^50, 2^51), its whole wave below 2^51
    assert sum(abs(int(v)) for v in C.first_episode_delta(pre, inp.alpha).ravel()) < 2 ** 62
    assert C.cost_operands_in_fast_range(pre, inp)
    name = "episode_sq16_kernel<16," if kernel == "auto" else "episode_kernel<16,"
    eng, ob = C.engine_for(inp, 1, q_dtype, battery=False), C.oracle_for(inp, 1, q_dtype, battery=False)
    for e in range(3):
        _episode(eng, ob, ("wide", q_dtype, kernel, e), name + q_dtype, episode=e, eps=0.6, battery=False, kernel=kernel)
    _episode(eng, ob, ("wide", q_dtype, kernel, "greedy"), name + q_dtype, mode="greedy", battery=False, kernel=kernel)
    eng.close()


# ----------------------------------------------------------------------------- C. short and odd horizons
def _short_inputs(T, seed=13):
    """S = 6: one full sq16 wave and half of one."""
    from p2pmicrogrid_amd.dataset import scenario_batch
    S, N = 6, 16
    inp = scenario_batch(S, N, T, seed=seed)
    return C.CaseInputs(np.broadcast_to(inp.time, (S, T)).copy(), inp.t_out, inp.load_w, inp.pv_w, inp.max_in, inp.t_in0,
                        inp.t_m0, C.hp_levels_for(S, N), np.full((S, N), C.BATTERY_J))


@pytest.mark.parametrize("philox_at", ["auto", "prepass"])
@pytest.mark.parametrize("R", [0, 1])
@pytest.mark.parametrize("T", [1, 2, 3, 7, 9])
def test_sq16_short_and_odd_horizons_match_oracle(T, R, philox_at):
    """episode_sq16_kernel where its step indices wrap at once: T = 1 and 2 alias the step words of
    steps t, t + 1 and t + 2; with R + 1 = 2 and in-kernel draws (philox="auto") one Philox block serves
    an even step and the odd one after it, and at odd T the last step is an even one whose block's second
    half no step uses.  (The code word the last iteration forms for the wrapped step 0 feeds only a row
    prefetch that nothing reads: taking the wrong half there changes no result, so no test can see it.)
    philox="prepass" has a pre-pass write the Philox code words, which the kernel
    then reads at the wrapped step index like uploaded ones.  Battery on for R = 1, off for R = 0; the second episode ends with the T0
    reset, the third records only {reward, cost}."""
    battery = R == 1
    inp = _short_inputs(T)
    eng, ob = C.engine_for(inp, R, battery=battery), C.oracle_for(inp, R, battery=battery)
    name = f"episode_sq16_kernel<16,f32,R1={R + 1},"
    for e in range(3):
        _episode(eng, ob, ("short", T, R, philox_at, e), name + "train", episode=e, eps=0.5, battery=battery,
                 record=NARROW if e == 2 else REC, reset_sigma=0.3 if e == 1 else None, philox=philox_at)
    _episode(eng, ob, ("short", T, R, philox_at, "greedy"), name + "greedy", mode="greedy", battery=battery)
    eng.close()


@pytest.mark.parametrize("R", [0, 1])
@pytest.mark.parametrize("T", [9, 12])
def test_sq16_replay_codes_match_oracle(T, R):
    """episode_sq16_kernel with uploaded exploration codes (rng = replay: the code words come from the
    codes buffer at the wrapped step index): two episodes with fresh codes each, about 40 % of the
    entries an action and the rest greedy, the delta applied in between."""
    battery = R == 1
    inp = _short_inputs(T, seed=17)
    eng, ob = C.engine_for(inp, R, battery=battery), C.oracle_for(inp, R, battery=battery)
    rs = np.random.RandomState(100 * T + R)
    for e in range(2):
        codes = C.replay_codes(rs, T, R, inp.S, inp.N)
        _episode(eng, ob, ("replay", T, R, e), f"episode_sq16_kernel<16,f32,R1={R + 1},train", rng="replay", episode=e,
                 codes=codes, battery=battery)
    eng.close()
