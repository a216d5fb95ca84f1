"""The device day profile without a device: the C ABI's two symbols and argument struct, and the library's host
planning (csrc/p2pmg_dayprof.cpp: validation, P and G, the 2^24 bound, launch shapes) with the number maps the
kernels share (p2pmg_dayprof.h: fix, the ordered-u32 image of an f32), driven by the stand-alone
tests/dayprof_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer.

What "every (group, slot) is covered exactly once" means for a launch shape (checked by the program): the step
slices partition the step range, and inside a slice every step has one row slot of the LDS tile, shared by
two steps only when they share t % P, so each (group, slot) a slice touches has exactly one row of its tile;
no tile exceeds the budget, and the global fallback is taken exactly when one slot of every group does not
fit."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import day_profile_ref as ref
from conftest import ROOT, TESTS

NEW = ("p2pmg_day_profile_shape", "p2pmg_day_profile")


def test_symbols_exported_with_argtypes_and_no_abi_bump():
    from p2pmicrogrid_amd import _lib
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        f = getattr(L, name)
        assert f.argtypes is not None and f.argtypes[0] is C.c_void_p and f.restype is C.c_int, name
    assert len(L.p2pmg_day_profile_shape.argtypes) == 4 and len(L.p2pmg_day_profile.argtypes) == 6
    assert L.p2pmg_abi_version() == 9 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "p2pmg.h")).read()
    assert "typedef struct p2pmg_day_profile_args {" in hdr
    assert all(f"int {name}(p2pmg_ctx* ctx, const p2pmg_day_profile_args* args" in hdr for name in NEW)
    bump = next(line for line in hdr.splitlines() if line.startswith("#define P2PMG_ABI_VERSION 9"))
    assert all(name in bump.split("added since without a bump")[1] for name in NEW)
    # null context: refused before anything is touched
    args = _lib.DayProfileArgs()
    assert L.p2pmg_day_profile_shape(None, C.byref(args), None, None) == 1
    assert L.p2pmg_day_profile(None, C.byref(args), None, None, None, None) == 1


@functools.lru_cache(maxsize=None)
def _check_output():
    """csrc/p2pmg_dayprof.cpp has no HIP call: it is compiled here with tests/dayprof_check.cpp as a program of
    its own, with -fsanitize=address,undefined, and run once.  The program opens no HIP device."""
    import tempfile
    from p2pmicrogrid_amd import _build
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dayprof_check")
        cmd = [_build.hipcc(), f"--offload-arch={_build.ARCH}", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-g",
               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
               f"-I{os.path.join(ROOT, 'include')}", f"-I{_build.CSRC}",
               os.path.join(_build.CSRC, "p2pmg_dayprof.cpp"), os.path.join(TESTS, "dayprof_check.cpp"), "-o", exe]
        built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert built.returncode == 0, built.stdout + built.stderr
        ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-4000:]
    return ran.stdout.splitlines()


def test_validation_bound_plans_and_maps_under_sanitizers():
    lines = _check_output()
    assert lines[-1].startswith("ok "), lines[-5:]
    assert int(lines[-1].split()[1]) >= 5000  # arguments, the bound, every launch shape of the sweep, fix, the image
    assert not [line for line in lines if line.startswith("FAILED")]


def test_struct_layout_matches_the_compiler():
    from p2pmicrogrid_amd import _lib
    sizes = [int(x) for x in _check_output()[0].split()[1:]]
    A = _lib.DayProfileArgs
    assert sizes == [C.sizeof(A)] + [getattr(A, n).offset for n, _ in A._fields_]
    assert [n for n, _ in A._fields_] == ["period", "step_first", "step_count", "scen_first", "scen_count", "n_groups", "groups"]


def test_fix_equals_the_reference_value_for_value():
    rows = [line.split() for line in _check_output() if line.startswith("fix ")]
    assert len(rows) >= 4000
    bits = np.array([int(r[1], 16) for r in rows], np.uint32)
    shift = np.array([int(r[2]) for r in rows])
    got = np.array([int(r[3]) for r in rows], np.int64)
    x = bits.view(np.float32)
    for k in (16, 24, 28):
        m = shift == k
        assert m.sum() > 1000 and np.array_equal(got[m], ref.fix(x[m], k)), k
        assert np.abs(x[m]).max() < 2.0 ** {16: 23, 24: 15, 28: 11}[k]
        assert (np.rint(x[m].astype(np.float64) * 2.0 ** k) != x[m].astype(np.float64) * 2.0 ** k).sum() > 50  # rounding happens
    assert (got < 0).sum() > 500 and (got == 0).sum() >= 3
