"""The build's unit table and header list cover csrc/ exactly: needs_build() and the object-freshness
check read them, so a source or header missing from them means a stale library."""
import os

from p2pmicrogrid_amd import _build


def test_unit_table_and_headers_cover_csrc():
    listed = {u[0] for u in _build.UNITS} | {h for h in _build.HEADERS if not os.path.isabs(h)}
    on_disk = {f for f in os.listdir(_build.CSRC) if f.endswith((".hip", ".cpp", ".h"))}
    assert on_disk == listed  # nothing unlisted, nothing listed that is gone
    assert all(os.path.isfile(h) for h in _build.HEADERS if os.path.isabs(h))


def test_monolithic_kernel_file_is_gone():
    assert not os.path.exists(os.path.join(_build.CSRC, "p2pmg_kernels.hip"))
