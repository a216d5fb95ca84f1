"""How many chained episodes per wave the launch planner chooses (csrc/p2pmg_plan.cpp): four, two or the
serial chain, by horizon, hazard distance, chain length and override.  tests/plan_check_groups.cpp holds
the cases; this test compiles it against the planner translation unit alone, as test_cpu_plan.py does
with plan_check.cpp, and runs it.  The program opens no HIP device."""
import os
import subprocess

from conftest import ROOT, TESTS


def test_planner_group_cases(tmp_path):
    from p2pmicrogrid_amd import _build
    exe = str(tmp_path / "plan_check_groups")
    cmd = [_build.hipcc(), f"--offload-arch={_build.ARCH}", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
           f"-I{os.path.join(ROOT, 'include')}", f"-I{_build.CSRC}",
           os.path.join(_build.CSRC, "p2pmg_plan.cpp"), os.path.join(TESTS, "plan_check_groups.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("ok "), ran.stdout
    assert int(ran.stdout.split()[1]) >= 40
