"""Policy sets without a GPU: the C ABI's new symbols, the host-side argument check
(csrc/p2pmg_host.cpp::validate_policy_set through the stand-alone tests/policy_set_check.cpp), the default and
snapshot maps, and the claim the GPU tests stand on: the oracle's greedy run reads its tables only through the
argmax, and the argmax of a policy's one-hot table is the policy's action."""
import os
import subprocess

import numpy as np
import pytest

import policy_set_ref as ref
from conftest import ROOT, TESTS

E_INVALID = 1  # P2PMG_E_INVALID (include/p2pmg.h)
NEW = ("p2pmg_set_policy_set", "p2pmg_get_policy_set", "p2pmg_policy_set_capture", "p2pmg_run_policy",
       "p2pmg_run_policy_ex")


def test_new_symbols_and_abi():
    from p2pmicrogrid_amd import _lib
    L = _lib.lib()
    assert L.p2pmg_abi_version() == 9 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "p2pmg.h")).read()
    for s in NEW:
        assert hasattr(L, s) and s in _lib.EXPORTS and f"int {s}(" in hdr, s
    assert [len(getattr(L, s).argtypes) for s in NEW] == [4, 4, 4, 2, 3]
    assert L.p2pmg_set_policy_set(None, 1, None, None) == E_INVALID
    assert L.p2pmg_get_policy_set(None, None, None, None) == E_INVALID
    assert L.p2pmg_policy_set_capture(None, 0, 0, 0) == E_INVALID
    assert L.p2pmg_run_policy(None, 0) == E_INVALID and L.p2pmg_run_policy_ex(None, 0, 0) == E_INVALID


def test_argument_checks_as_a_host_program(tmp_path):
    """validate_policy_set has no HIP call: compiled with tests/policy_set_check.cpp into a program of its own,
    with -fsanitize=address,undefined, and run.  The program opens no HIP device."""
    from p2pmicrogrid_amd import _build
    exe = str(tmp_path / "policy_set_check")
    cmd = [_build.hipcc(), f"--offload-arch={_build.ARCH}", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-g",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           f"-I{os.path.join(ROOT, 'include')}", f"-I{_build.CSRC}",
           os.path.join(_build.CSRC, "p2pmg_host.cpp"), os.path.join(TESTS, "policy_set_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("ok ") and int(ran.stdout.split()[1]) >= 100, ran.stdout


def test_default_map_arithmetic():
    from p2pmicrogrid_amd.engine import default_policy_map
    S, N = 5, 3
    assert np.array_equal(default_policy_map(15, S, N), np.arange(15))
    assert np.array_equal(default_policy_map(3, S, N), np.arange(15) % 3)
    assert np.array_equal(default_policy_map(1, S, N), np.zeros(15))
    assert default_policy_map(3, S, N).dtype == np.int32
    assert np.array_equal(default_policy_map(3, 1, 3), np.arange(3))  # M == A == N: the identity either way
    assert np.array_equal(default_policy_map(1, 4, 1), np.zeros(4))   # M == N == 1
    for m in (0, 2, 4, 14, 16):
        with pytest.raises(ValueError, match="needs policy_of"):
            default_policy_map(m, S, N)


def test_snapshot_map_and_the_shapes_evaluate_policies_builds():
    """K snapshots x D days are S = K * D scenarios; scenario k * D + d, agent i reads policy k * N + i."""
    from p2pmicrogrid_amd.engine import snapshot_policy_map
    K, D, N = 3, 4, 2
    m = snapshot_policy_map(K, D, N)
    assert m.shape == (K * D, N) and m.dtype == np.int32
    for k in range(K):
        for d in range(D):
            assert list(m[k * D + d]) == [k * N + i for i in range(N)]
    assert m.min() == 0 and m.max() == K * N - 1
    # the day inputs are tiled the same way: row k * D + d of a [D, ...] stack tiled K times is day d
    days = np.arange(D * 5).reshape(D, 5)
    tiled = np.tile(days, (K, 1))
    assert all(np.array_equal(tiled[k * D + d], days[d]) for k in range(K) for d in range(D))
    assert np.array_equal(np.repeat(np.arange(K), D), m[:, 0] // N)  # the profile's groups: the snapshot index


def test_evaluate_policies_reads_flat_bytes_on_the_agents_grid():
    """Flat bytes carry no grid: they are read on the agents' tables' grid and refused, before any device call
    and with the reason, when they do not fit it."""
    from p2pmicrogrid_amd import community
    from p2pmicrogrid_amd.agent import QAgent
    np.random.seed(42)
    com = community.get_community(QAgent, 2)
    days = [{"time": np.zeros(4, np.float32)}]
    small = np.zeros((1, 2, 6 * 5 * 7 * 4), np.uint8)
    with pytest.raises(ValueError, match=r"840 states do not fit the grid \(20, 20, 20, 20\) \(160000 states\)"):
        com.evaluate_policies(days, small)
    with pytest.raises(ValueError, match=r"n_time, n_temp, n_bal, n_p2p"):
        com.evaluate_policies(days, small.reshape(1, 2, 30, 28))
    with pytest.raises(ValueError, match="uint8"):
        com.evaluate_policies(days, small.astype(np.int64))
    assert com.evaluate_policies([], small) == [] and com.evaluate_policies(days, small[:0], profile=True) == ([], None)


def test_policy_bytes_is_the_flat_greedy_policy_unbound():
    from p2pmicrogrid_amd.rl import QActor
    rs = np.random.RandomState(3)
    act = QActor(6, 5, 7, 4, 3)
    q = np.zeros((6, 5, 7, 4, 3))
    rows = rs.rand(6, 5, 7, 4) < 0.4
    q[rows] = rs.randn(int(rows.sum()), 3)
    act.set_qtable(q)
    b = act.policy_bytes()
    assert b.dtype == np.uint8 and b.shape == (6 * 5 * 7 * 4,) and b.flags.c_contiguous
    assert np.array_equal(b, act.greedy_policy().reshape(-1))
    assert np.array_equal(b == 255, ~rows.reshape(-1))
    assert np.array_equal(ref.action_of(b), np.argmax(q.reshape(-1, 3), axis=-1))


def test_one_hot_argmax_is_the_policy_action():
    pol = ref.random_policies(7, 1000, seed=1)
    assert set(np.unique(pol)) == {0, 1, 2, 255}
    want = np.where(pol == 255, 0, pol)
    for alt in (False, True):
        q = ref.one_hot_tables(pol, alt=alt)
        assert np.array_equal(np.argmax(q, axis=-1), want)
        assert np.array_equal(q.any(axis=-1), pol != 255)  # visited exactly where the byte is an action
    assert np.array_equal(ref.action_of(pol), want)
    assert not np.array_equal(ref.one_hot_tables(pol), ref.one_hot_tables(pol, alt=True))


@pytest.mark.parametrize("N,R", [(2, 1), (3, 2)])
def test_oracle_greedy_depends_on_tables_only_through_the_packed_policy(N, R):
    """Two different table sets with the same packed policy give equal records, and a third with another
    policy does not: the oracle's greedy run is a function of the argmax alone."""
    S, T, dims = 3, 12, (6, 5, 7, 4)
    inp = ref.inputs(S, N, T)
    pol = ref.random_policies(S * N, int(np.prod(dims)), seed=2)
    a = ref.oracle_for(inp, N, R, ref.one_hot_tables(pol), dims=dims).run_episode("greedy")
    b = ref.oracle_for(inp, N, R, ref.one_hot_tables(pol, alt=True), dims=dims).run_episode("greedy")
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the actions taken are the policy's bytes at the visited rows
    it, iT, ib, ip = (a["idx"][..., j] for j in range(4))
    row = ((it * dims[1] + iT) * dims[2] + ib) * dims[3] + ip           # [T, R+1, S, N]
    agent = np.arange(S * N).reshape(S, N)
    assert np.array_equal(a["action"], ref.action_of(pol)[agent[None, None], row])
    assert len(np.unique(a["action"])) == 3 and len(np.unique(iT)) > 2
    other = ref.random_policies(S * N, int(np.prod(dims)), seed=3)
    c = ref.oracle_for(inp, N, R, ref.one_hot_tables(other), dims=dims).run_episode("greedy")
    assert not np.array_equal(a["action"], c["action"]) and not np.array_equal(a["cost"], c["cost"])
