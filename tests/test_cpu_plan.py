"""The launch planner (csrc/p2pmg_plan.cpp) decides which kernel family an episode launch gets, where
its Philox draws come from, its scenarios per wave and its record layout, as a pure function.
tests/plan_check.cpp asserts the choice for every configuration class the runtime distinguishes;
this test compiles it against the planner translation unit alone (no runtime, no kernels) with the
library's compiler and flags, and runs it.  The program opens no HIP device."""
import os
import subprocess

from conftest import ROOT, TESTS


def test_planner_cases(tmp_path):
    from p2pmicrogrid_amd import _build
    exe = str(tmp_path / "plan_check")
    cmd = [_build.hipcc(), f"--offload-arch={_build.ARCH}", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
           f"-I{os.path.join(ROOT, 'include')}", f"-I{_build.CSRC}",
           os.path.join(_build.CSRC, "p2pmg_plan.cpp"), os.path.join(TESTS, "plan_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("ok "), ran.stdout
    assert int(ran.stdout.split()[1]) >= 60
