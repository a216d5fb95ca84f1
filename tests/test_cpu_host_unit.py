"""The runtime's HIP-free unit (csrc/p2pmg_host.cpp) as a program of its own: the config check p2pmg_create
makes before its first device call, the default config and the replay decoder, driven by the stand-alone
tests/host_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

from conftest import ROOT, TESTS


def test_host_unit_includes_no_hip_header():
    from p2pmicrogrid_amd import _build
    for name in ("p2pmg_host.cpp", "p2pmg_host.h"):
        txt = open(os.path.join(_build.CSRC, name)).read()
        inc = re.findall(r'#include\s+[<"]([^>"]+)[>"]', txt)
        assert inc and not [i for i in inc if "hip" in i or i in ("p2pmg_internal.h", "p2pmg_ctx.h")], (name, inc)


def test_host_unit_under_sanitizers(tmp_path):
    """csrc/p2pmg_host.cpp has no HIP call: it is compiled here with tests/host_check.cpp as a program of its
    own, with -fsanitize=address,undefined, and run.  The program opens no HIP device."""
    from p2pmicrogrid_amd import _build
    exe = str(tmp_path / "host_check")
    cmd = [_build.hipcc(), f"--offload-arch={_build.ARCH}", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-g",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           f"-I{os.path.join(ROOT, 'include')}", f"-I{_build.CSRC}",
           os.path.join(_build.CSRC, "p2pmg_host.cpp"), os.path.join(TESTS, "host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("ok "), ran.stdout
    assert int(ran.stdout.split()[1]) >= 67
