"""Per-agent learner constants and per-scenario epsilon, the parts that need no GPU: the new symbols
(ABI still 9), the planner's two facts (tests/plan_check_learning.cpp, compiled against the planner
translation unit alone), community.learning_arrays, and the shapes the Python layer refuses."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT, TESTS
from p2pmicrogrid_amd import _lib
from p2pmicrogrid_amd.community import learning_arrays
from p2pmicrogrid_amd.engine import DeviceCommunityBatch
from p2pmicrogrid_amd.rl import QActor

NEW = ("p2pmg_set_learning", "p2pmg_get_learning", "p2pmg_run_episodes_eps")


def test_abi_version_and_new_symbols():
    assert _lib.ABI_VERSION == 9
    L = _lib.lib()
    assert L.p2pmg_abi_version() == 9
    header = open(os.path.join(ROOT, "include", "p2pmg.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(" in header, name
    # null contexts are refused, not dereferenced
    assert L.p2pmg_set_learning(None, None, None, None) == 1
    assert L.p2pmg_get_learning(None, None, None, None) == 1


def test_planner_learning_facts(tmp_path):
    from p2pmicrogrid_amd import _build
    exe = str(tmp_path / "plan_check_learning")
    cmd = [_build.hipcc(), f"--offload-arch={_build.ARCH}", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
           f"-I{os.path.join(ROOT, 'include')}", f"-I{_build.CSRC}",
           os.path.join(_build.CSRC, "p2pmg_plan.cpp"), os.path.join(TESTS, "plan_check_learning.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("ok "), ran.stdout
    assert int(ran.stdout.split()[1]) >= 40


def test_learning_arrays():
    agents = [SimpleNamespace(actor=QActor(20, 20, 20, 20, alpha=1e-3, gamma=0.5)),
              SimpleNamespace(actor=QActor(20, 20, 20, 20)),
              SimpleNamespace(actor=QActor(20, 20, 20, 20, alpha=0.5, gamma=0.0))]
    alpha, gamma = learning_arrays(agents)
    assert alpha.dtype == np.float64 and gamma.dtype == np.float64
    assert np.array_equal(alpha, [1e-3, 1e-5, 0.5]) and np.array_equal(gamma, [0.5, 0.9, 0.0])
    agents[1].actor._alpha = 0.25
    assert np.array_equal(learning_arrays(agents)[0], [1e-3, 0.25, 0.5])


class _Shapes(DeviceCommunityBatch):
    """The argument checks of set_learning / run_episodes / run_episode run before any library call:
    an instance with the sizes alone, whose library handle refuses to be used."""

    def __init__(self, S, N):  # noqa: super().__init__ would create a device context
        self.S, self.N, self.A = S, N, S * N
        self._ctx = None

    @property
    def L(self):
        raise AssertionError("the shape check must come before the library call")

    def close(self):
        pass


def test_python_rejects_wrong_shapes():
    eng = _Shapes(3, 4)
    for kw in (dict(alpha=np.zeros((4, 3))), dict(gamma=np.zeros(5)), dict(penalty_weight=np.zeros((2, 3, 4)))):
        with pytest.raises(ValueError, match="broadcast"):
            eng.set_learning(**kw)
    for eps in (np.zeros((2, 4)), np.zeros((2, 3, 1)), np.zeros((0, 3))):
        with pytest.raises(ValueError, match="epsilons"):
            eng.run_episodes(0, eps)
    with pytest.raises(ValueError, match="epsilon"):
        eng.run_episode("train", "philox", epsilon=np.zeros(4))
    with pytest.raises(ValueError, match="philox"):
        eng.run_episode("train", "replay", epsilon=np.zeros(3))
    with pytest.raises(ValueError, match="philox"):
        eng.run_episode("greedy", epsilon=np.zeros(3))
