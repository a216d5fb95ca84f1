"""Per-network DQN learner constants without a GPU: the C ABI's new symbols and prototypes, the host-side
range check (csrc/p2pmg_host.cpp::validate_dqn_learning through the stand-alone tests/dqn_learning_check.cpp),
the mixed-value reference (tests/dqn_learning_ref.py) against OracleDQNBatch at equal values, and
ShardedTrainer's slicing of per-agent values and per-scenario epsilons."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TESTS
from oracle import dqn as odqn
from p2pmicrogrid_amd.dataset import scenario_batch

E_INVALID, E_STATE = 1, 4  # P2PMG_E_INVALID, P2PMG_E_STATE (include/p2pmg.h)
NEW = ("p2pmg_dqn_set_learning", "p2pmg_dqn_get_learning", "p2pmg_dqn_run_episode_eps")


def test_new_symbols_and_abi():
    from p2pmicrogrid_amd import _lib
    L = _lib.lib()
    assert L.p2pmg_abi_version() == 9 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "p2pmg.h")).read()
    for s in NEW:
        assert hasattr(L, s) and s in _lib.EXPORTS and f"int {s}(" in hdr, s
    assert len(L.p2pmg_dqn_set_learning.argtypes) == 6 and len(L.p2pmg_dqn_get_learning.argtypes) == 6
    assert len(L.p2pmg_dqn_run_episode_eps.argtypes) == 3
    assert L.p2pmg_dqn_set_learning(None, None, None, None, None, None) == E_INVALID
    assert L.p2pmg_dqn_get_learning(None, None, None, None, None, None) == E_INVALID
    args = _lib.EpisodeArgs(_lib.MODE_TRAIN, _lib.RNG_PHILOX, 0, 0, 0.5, 0, 0)
    assert L.p2pmg_dqn_run_episode_eps(None, C.byref(args), np.zeros(1)) == E_INVALID


def test_range_check_as_a_host_program(tmp_path):
    """validate_dqn_learning has no HIP call: compiled with tests/dqn_learning_check.cpp into a program of its
    own, with -fsanitize=address,undefined, and run.  The program opens no HIP device."""
    from p2pmicrogrid_amd import _build
    exe = str(tmp_path / "dqn_learning_check")
    cmd = [_build.hipcc(), f"--offload-arch={_build.ARCH}", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-g",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           f"-I{os.path.join(ROOT, 'include')}", f"-I{_build.CSRC}",
           os.path.join(_build.CSRC, "p2pmg_host.cpp"), os.path.join(TESTS, "dqn_learning_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("ok ") and int(ran.stdout.split()[1]) >= 20, ran.stdout


def _inputs(S, N, T):
    inp = scenario_batch(S, N, T)
    return dict(S=S, N=N, R=1, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in, env_time=inp.time[None],
                env_tout=inp.t_out, theta0=odqn.glorot_init(S * N, seed=5), dqn=odqn.DQNParams(capacity=64))


def test_reference_equals_oracle_at_equal_values():
    """Two fill episodes and one train episode at S = 2, N = 2, R = 1, T = 16: with the default values in
    every row the per-network reference is OracleDQNBatch bit for bit (records, rings, weights, Adam state)."""
    from dqn_learning_ref import MixedDQNBatch
    kw = _inputs(2, 2, 16)
    a, b = odqn.OracleDQNBatch(**kw), MixedDQNBatch(**kw)
    for ep, (mode, eps) in enumerate((("fill", 1.0), ("fill", 1.0), ("train", 0.6))):
        oa = a.run_episode(mode, rng="philox", episode=ep, eps=eps)
        ob = b.run_episode(mode, rng="philox", episode=ep, eps=eps)
        for k in oa:
            assert np.array_equal(oa[k], ob[k]), (ep, k)
    for k in ("theta", "target", "m", "v", "buf", "added", "t_in", "t_m"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert not np.array_equal(a.theta, kw["theta0"]) and odqn.soft_update is not None
    g = b.get_learning()
    assert (g["gamma"] == 0.95).all() and (g["tau"] == 0.005).all() and (g["lr"] == 1e-5).all() and (g["clip"] == 1).all()
    assert (g["penalty_weight"] == 10).all()


def test_per_scenario_eps_equals_one_launch_per_rate():
    """per_scenario_eps(): scenario s of one batch at eps[s] is the S = 1 oracle run of that scenario's global
    agent ids at the scalar eps[s], bit for bit (0.002 < 2^-8 takes the small-epsilon action layout)."""
    from dqn_learning_ref import per_scenario_eps
    S, N, T = 3, 2, 16
    kw, eps = _inputs(S, N, T), np.array([0.002, 0.7, 1.0])
    whole = odqn.OracleDQNBatch(**kw)
    with per_scenario_eps():
        got = whole.run_episode("fill", rng="philox", episode=1, eps=eps[:, None])
    assert odqn.philox.launch_eps([0.5, 0.5]) == 0.5  # the hook is gone
    for s in range(S):
        k1 = dict(kw, S=1, load_w=kw["load_w"][s:s + 1], pv_w=kw["pv_w"][s:s + 1], max_in=kw["max_in"][s:s + 1],
                  env_tout=kw["env_tout"][s:s + 1], theta0=kw["theta0"][s * N:(s + 1) * N])
        one = odqn.OracleDQNBatch(**k1)
        want = one.run_episode("fill", rng="philox", episode=1, eps=float(eps[s]), agent_ids=np.arange(s * N, (s + 1) * N))
        for k in ("action", "reward", "cost", "t_in"):
            assert np.array_equal(got[k][..., s:s + 1, :], want[k]), (s, k)
        assert np.array_equal(whole.buf[s], one.buf[0])


def test_reference_rows_differ_and_restore():
    """A row with other values changes that network alone; set_learning() restores the constructor's."""
    from dqn_learning_ref import MixedDQNBatch
    kw = _inputs(1, 2, 16)
    a, b = MixedDQNBatch(**kw), MixedDQNBatch(**kw)
    b.set_learning(gamma=[[0.95, 0.5]], lr=[[1e-5, 1e-3]], penalty_weight=[[10.0, 3.0]])
    for ob in (a, b):
        for ep, mode in enumerate(("fill", "fill", "train")):
            ob.run_episode(mode, rng="philox", episode=ep, eps=1.0)
    assert np.array_equal(a.theta[0], b.theta[0]) and not np.array_equal(a.theta[1], b.theta[1])
    b.set_learning()
    assert [d.gamma for d in b.net_dqn] == [0.95, 0.95] and b.params.penalty_weight == 10.0


class _FakeEngine:
    """What ShardedTrainer calls on its engine, recorded (the fake engine_factory of test_cpu_role_tables)."""

    def __init__(self, S, N, shared):
        self.S, self.N, self.shared, self.calls = S, N, shared, []

    def set_learning(self, gamma=None, tau=None, lr=None, clip=None, penalty_weight=None):
        self.calls.append(("set_learning", gamma, tau, lr, clip, penalty_weight))

    def run_episode(self, mode, rng, episode=0, epsilon=1.0, **kw):
        self.calls.append((mode, episode, epsilon))

    def episode_reward(self):
        return np.zeros(self.S, np.float32)

    def __getattr__(self, name):  # set_env, set_profiles, set_max_in, set_temperatures, reset_temperatures_philox
        return lambda *a, **k: None


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("shared", [True, False])
def test_sharded_trainer_slices_by_scenario_range(rank, shared):
    from p2pmicrogrid_amd.distributed import ShardedTrainer, shard
    S, N, world = 6, 2, 2
    made = {}

    def factory(sh, S_, N_, R, T, q_dtype, device, seed, shared_q=False, **dqn):
        made["eng"] = _FakeEngine(S_, N_, shared)
        return made["eng"]
    tr = ShardedTrainer(S, N, 1, 16, rank=rank, world=1, engine_factory=factory, learner="dqn")
    tr.sh, tr.world = shard(S, rank, world), world  # the rank's shard, without a process group
    tr.exchange = None
    lo, hi = tr.sh.first, tr.sh.first + tr.sh.count
    w = np.arange(S * N, dtype=np.float32).reshape(S, N)
    gamma = np.linspace(0.5, 0.9, S * N).reshape(S, N)
    tr.set_learning(gamma=0.9 if shared else gamma, tau=0.01, penalty_weight=w)
    _, g, t, lr, clip, pw = made["eng"].calls[-1]
    assert np.array_equal(pw, w[lo:hi]) and lr is None and clip is None
    if shared:
        assert g == 0.9 and t == 0.01            # the one row, unchanged on every rank
    else:
        assert np.array_equal(g, gamma[lo:hi]) and np.array_equal(t, np.full((hi - lo, N), 0.01))
    eps = np.linspace(0.1, 0.6, S)
    tr.filled = True
    tr._metrics = lambda: (0.0, 1.0)
    tr.train_episode(eps)
    mode, episode, got = made["eng"].calls[-1]
    assert mode == "train" and np.array_equal(got, eps[lo:hi])
    tr.train_episode(0.25)
    assert made["eng"].calls[-1][2] == 0.25
    with pytest.raises(ValueError):
        tr.train_episode(eps[:-1])
    tab = ShardedTrainer(2, 2, 0, 12, engine_factory=lambda *a, **k: _FakeEngine(2, 2, False))
    with pytest.raises(ValueError):
        tab.set_learning(gamma=0.9)
