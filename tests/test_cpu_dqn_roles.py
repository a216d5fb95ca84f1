"""One DQN network per role without a GPU: the C ABI's two new symbols, the host-side argument checks
(csrc/p2pmg_host.cpp::validate_dqn_roles through the stand-alone tests/dqn_roles_check.cpp), the role reference
(tests/dqn_role_ref.py) against OracleDQNBatch at N = 1 (the shared network) and S = 1 (per-agent networks),
and the Python argument check of DeviceDQNBatch(shared=...)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TESTS
from oracle import dqn as odqn
from p2pmicrogrid_amd.dataset import scenario_batch

E_INVALID = 1  # P2PMG_E_INVALID (include/p2pmg.h)
NEW = ("p2pmg_dqn_setup_roles", "p2pmg_dqn_roles")
T, CAP, HELD = 12, 64, 40  # 40 transitions preloaded + one fill of 12: training is admitted; 76 > 64 evicts


def test_new_symbols_and_abi():
    from p2pmicrogrid_amd import _lib
    L = _lib.lib()
    assert L.p2pmg_abi_version() == 9 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "p2pmg.h")).read()
    for s in NEW:
        assert hasattr(L, s) and s in _lib.EXPORTS and f"int {s}(" in hdr, s
    assert len(L.p2pmg_dqn_setup_roles.argtypes) == 2 and len(L.p2pmg_dqn_roles.argtypes) == 2
    assert L.p2pmg_dqn_setup_roles(None, None) == E_INVALID
    assert L.p2pmg_dqn_roles(None, None) == E_INVALID
    assert "no per-role network is TRAINED" not in hdr and "p2pmg_dqn_setup_roles is the route" in hdr


def test_argument_checks_as_a_host_program(tmp_path):
    """validate_dqn_roles has no HIP call: compiled with tests/dqn_roles_check.cpp into a program of its own,
    with -fsanitize=address,undefined, and run.  The program opens no HIP device."""
    from p2pmicrogrid_amd import _build
    exe = str(tmp_path / "dqn_roles_check")
    cmd = [_build.hipcc(), f"--offload-arch={_build.ARCH}", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-g",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           f"-I{os.path.join(ROOT, 'include')}", f"-I{_build.CSRC}",
           os.path.join(_build.CSRC, "p2pmg_host.cpp"), os.path.join(TESTS, "dqn_roles_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("ok ") and int(ran.stdout.split()[1]) >= 30, ran.stdout


def _inputs(S, N):
    inp = scenario_batch(S, N, T)
    return dict(S=S, N=N, R=1, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in, env_time=inp.time[None],
                env_tout=inp.t_out, dqn=odqn.DQNParams(capacity=CAP))


def _run_pair(a, b):
    """A fill episode and two training episodes on both; every record, then the whole state, must be equal."""
    from dqn_role_ref import load_rings, preload_rings
    ring, added = preload_rings(a.S * a.N, CAP, HELD)
    for ob in (a, b):
        load_rings(ob, ring, added)
    for ep, (mode, eps) in enumerate((("fill", 1.0), ("train", 0.6), ("train", 0.3))):
        oa = a.run_episode(mode, rng="philox", episode=ep, eps=eps)
        ob = b.run_episode(mode, rng="philox", episode=ep, eps=eps)
        for k in oa:
            assert np.array_equal(oa[k], ob[k]), (ep, k)
        assert mode == "fill" or oa["loss"].all()
    for k in ("theta", "target", "m", "v"):
        assert np.array_equal(getattr(a, k).reshape(-1), getattr(b, k).reshape(-1)), k
    for k in ("buf", "added", "t_in", "t_m"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert int(a.added.min()) == HELD + 3 * T > CAP and a.step == b.step == 2 * T


def test_reference_with_one_role_is_the_shared_network(apb=2):
    """N = 1, S = 5: blocks of 2, 2, 1 agents at agents_per_block = 2, the same in both."""
    from dqn_role_ref import RoleDQNBatch
    kw = _inputs(5, 1)
    theta0 = odqn.glorot_init(1, seed=5)
    a = odqn.OracleDQNBatch(**kw, theta0=theta0, shared=True, agents_per_block=apb)
    b = RoleDQNBatch(**kw, theta0=theta0, agents_per_block=apb)
    assert b.theta.shape == (1, odqn.N_PARAMS)
    _run_pair(a, b)
    assert not np.array_equal(a.theta, theta0)


def test_reference_with_one_scenario_is_per_agent_networks():
    """S = 1, N = 3: every role has one agent, one block, one partial; the sum of one partial and zeros times 1 / 1
    is the per-agent gradient."""
    from dqn_role_ref import RoleDQNBatch
    kw = _inputs(1, 3)
    theta0 = odqn.glorot_init(3, seed=5)
    a = odqn.OracleDQNBatch(**kw, theta0=theta0)
    b = RoleDQNBatch(**kw, theta0=theta0, agents_per_block=4)
    assert b.theta.shape == (3, odqn.N_PARAMS) and b.m.shape == b.v.shape == b.target.shape == (3, odqn.N_PARAMS)
    _run_pair(a, b)


def test_reference_roles_learn_apart_and_take_their_own_rows():
    """S = 2, N = 2: the two networks end apart from each other; a row with another lr and tau changes that role
    alone; set_learning() restores the constructor's values."""
    from dqn_role_ref import RoleDQNBatch, load_rings, preload_rings
    kw = _inputs(2, 2)
    theta0 = np.repeat(odqn.glorot_init(1, seed=5), 2, axis=0)  # both roles start from the same weights
    a, b = RoleDQNBatch(**kw, theta0=theta0), RoleDQNBatch(**kw, theta0=theta0)
    b.set_learning(lr=[1e-5, 1e-3], tau=[0.005, 0.5])
    assert b.get_learning()["lr"].shape == (2,) and b.get_learning()["penalty_weight"].shape == (2, 2)
    ring, added = preload_rings(4, CAP, HELD)
    for ob in (a, b):
        load_rings(ob, ring, added)
        ob.run_episode("train", rng="philox", episode=0, eps=0.5)
    assert not np.array_equal(a.theta[0], a.theta[1])
    # role 1's own lr (100 x) and tau: its weights move about 100 x as far from the start, role 0's as far as before
    # (not to the bit: the two roles trade with each other, so role 0's transitions change with role 1's policy)
    d = lambda ob, i: float(np.abs(ob.theta[i].astype(np.float64) - theta0[i]).max())  # noqa: E731
    assert 30 * d(a, 1) < d(b, 1) < 300 * d(a, 1) and 0.5 * d(a, 0) < d(b, 0) < 2 * d(a, 0)
    gap = lambda ob, i: float(np.abs(ob.theta[i].astype(np.float64) - ob.target[i]).max())  # noqa: E731
    assert gap(b, 1) < 0.3 * d(b, 1) and gap(a, 1) > 0.5 * d(a, 1)  # tau 0.5 keeps the target next to the online net
    b.set_learning()
    assert [d.lr for d in b.role_dqn] == [1e-5, 1e-5]
    with pytest.raises(ValueError):
        RoleDQNBatch(**kw, theta0=odqn.glorot_init(4, seed=5))
    assert odqn.soft_update.__module__ == "oracle.dqn"  # the hook is gone


def test_python_refuses_other_strings():
    from p2pmicrogrid_amd.dqn import DeviceDQNBatch
    with pytest.raises(ValueError, match="role"):
        DeviceDQNBatch(2, 2, 1, T, shared="roles")
    with pytest.raises(ValueError):
        DeviceDQNBatch(2, 2, 1, T, shared="")
