"""Sparse table checkpoints without a device: the C ABI's four symbols, the NumPy statement of the format
(rl.sparse_table / rl.dense_table), the file format, an unbound QActor's save_sparse / load_sparse, and the
library's host validation and run planning (csrc/p2pmg_sparse.cpp) driven by the stand-alone
tests/sparse_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import numpy as np
import pytest

import sparse_table_ref as ref
from conftest import ROOT, TESTS

NEW = ("p2pmg_sparse_count", "p2pmg_get_q_sparse", "p2pmg_set_q_sparse", "p2pmg_copy_q")
SHAPE = (3, 4, 5, 2, 3)


def test_symbols_exported_with_argtypes_and_no_abi_bump():
    import ctypes as C
    from p2pmicrogrid_amd import _lib
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        f = getattr(L, name)
        assert f.argtypes is not None and f.argtypes[0] is C.c_void_p and f.restype is C.c_int, name
    assert len(L.p2pmg_sparse_count.argtypes) == 4 and len(L.p2pmg_get_q_sparse.argtypes) == 8
    assert L.p2pmg_get_q_sparse.argtypes[3] is C.c_int64
    assert len(L.p2pmg_set_q_sparse.argtypes) == 8 and len(L.p2pmg_copy_q.argtypes) == 4
    assert L.p2pmg_abi_version() == 9 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "p2pmg.h")).read()
    assert "#define P2PMG_SPARSE_STAGE_BYTES (8u << 20)" in hdr and _lib.SPARSE_STAGE_BYTES == 8 << 20
    bump = next(line for line in hdr.splitlines() if line.startswith("#define P2PMG_ABI_VERSION 9"))
    assert all(name in bump.split("added since without a bump")[1] for name in NEW)
    # null context: refused before anything is touched
    assert L.p2pmg_sparse_count(None, 0, 1, None) == 1 and L.p2pmg_copy_q(None, 0, 1, 1) == 1
    assert L.p2pmg_get_q_sparse(None, 0, 1, 0, None, None, None, 0) == 1
    assert L.p2pmg_set_q_sparse(None, 0, 1, None, None, None, 0, 1) == 1


@pytest.mark.parametrize("q", ["f64", "f32"])
def test_sparse_and_dense_round_trip_byte_for_byte(q):
    from p2pmicrogrid_amd import rl
    n_states = int(np.prod(SHAPE[:-1]))
    t = ref.tables(4, n_states, 3, q, seed=8)
    sp = rl.sparse_table(t.reshape(4, *SHAPE))
    n_rows, rows, values = ref.sparse(t)
    assert sp["shape"].dtype == np.int64 and tuple(sp["shape"]) == SHAPE
    assert sp["offsets"].dtype == np.int64 and np.array_equal(np.diff(sp["offsets"]), n_rows) and sp["offsets"][0] == 0
    assert sp["rows"].dtype == np.int32 and np.array_equal(sp["rows"], rows)
    assert sp["values"].dtype == t.dtype and np.array_equal(ref.bits(sp["values"]), ref.bits(values))
    # -0.0 rows are stored although nothing in them is != 0; table 1 is empty, table 2 complete
    neg = np.flatnonzero(ref.stored(t[0:1])[0] & ~(t[0] != 0).any(axis=-1))
    assert len(neg) >= 3 and np.isin(neg, sp["rows"][:n_rows[0]]).all()
    assert n_rows[1] == 0 and n_rows[2] == n_states and 0 < n_rows[0] < n_states
    back = rl.dense_table(sp)
    assert back.dtype == t.dtype and back.shape == (4, *SHAPE)
    assert np.array_equal(ref.bits(back.reshape(t.shape)), ref.bits(t))
    one = rl.sparse_table(t[0].reshape(SHAPE))  # one table: count = 1
    assert one["offsets"].tolist() == [0, n_rows[0]]
    assert np.array_equal(ref.bits(rl.dense_table(one)[0].reshape(-1, 3)), ref.bits(t[0]))


def test_dense_table_refuses_what_is_no_sparse_form():
    from p2pmicrogrid_amd import rl
    good = rl.sparse_table(ref.tables(2, 120, 3, "f64").reshape(2, *SHAPE))
    rl.dense_table(good)
    for key, bad in (("rows", good["rows"][::-1]), ("rows", np.where(np.arange(len(good["rows"])) == 1, good["rows"][0],
                                                                    good["rows"])),
                     ("rows", good["rows"] + 120), ("rows", good["rows"] - 121), ("offsets", good["offsets"] + 1),
                     ("offsets", good["offsets"][:1]), ("values", good["values"][:, :2]), ("shape", good["shape"][:4])):
        with pytest.raises(ValueError):
            rl.dense_table({**good, key: bad})
    with pytest.raises(ValueError):
        rl.dense_table({k: v for k, v in good.items() if k != "rows"})


def test_unbound_actor_saves_and_loads_the_file_format(tmp_path):
    from p2pmicrogrid_amd import rl
    t = ref.tables(1, 120, 3, "f64", seed=4)[0].reshape(SHAPE)
    a = rl.QActor(*SHAPE[:-1])
    a.set_qtable(t)
    path = str(tmp_path / "actor.npz")
    a.save_sparse(path)
    assert a._engine is None  # no device was taken
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == ["offsets", "rows", "shape", "values"]
        assert f["shape"].dtype == np.int64 and tuple(f["shape"]) == SHAPE
        assert f["offsets"].dtype == np.int64 and f["offsets"].shape == (2,)
        assert f["rows"].dtype == np.int32 and f["values"].dtype == np.float64
        assert f["values"].shape == (len(f["rows"]), 3) and f["offsets"][1] == len(f["rows"])
        n_rows, rows, values = ref.sparse(t.reshape(1, -1, 3))
        assert np.array_equal(f["rows"], rows) and np.array_equal(ref.bits(f["values"]), ref.bits(values))
    import zipfile
    with zipfile.ZipFile(path) as z:  # uncompressed
        assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())
    b = rl.QActor(*SHAPE[:-1])
    b.set_qtable(np.ones(SHAPE))  # every row the file does not list becomes zero
    b.load_sparse(path)
    assert b._engine is None and np.array_equal(ref.bits(b.q_table), ref.bits(t))
    with pytest.raises(ValueError):
        rl.QActor(3, 4, 5, 3).load_sparse(path)  # another table shape
    rl.save_sparse_file(str(tmp_path / "two"), rl.sparse_table(np.zeros((2, *SHAPE))))  # ".npz" is appended
    with pytest.raises(ValueError):
        b.load_sparse(str(tmp_path / "two.npz"))  # two tables are no actor's
    with pytest.raises(ValueError):
        rl.load_sparse_file(path, shape=(3, 4, 5, 2, 2))


def test_host_validation_and_run_planning_under_sanitizers(tmp_path):
    """csrc/p2pmg_sparse.cpp has no HIP call: it is compiled here with tests/sparse_check.cpp as a program
    of its own, with -fsanitize=address,undefined, and run.  The program opens no HIP device."""
    from p2pmicrogrid_amd import _build
    exe = str(tmp_path / "sparse_check")
    cmd = [_build.hipcc(), f"--offload-arch={_build.ARCH}", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-g",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           f"-I{os.path.join(ROOT, 'include')}", f"-I{_build.CSRC}",
           os.path.join(_build.CSRC, "p2pmg_sparse.cpp"), os.path.join(TESTS, "sparse_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("ok "), ran.stdout
    assert int(ran.stdout.split()[1]) >= 230
