"""Drive the sparse table checkpoints and get_q's device pass over the same tables, for a kernel trace
(profiles/sparse_tables/README.md):

    rocprofv3 --kernel-trace --stats -d <dir> -o sp --output-format csv -- \\
        python scripts/sparse_tables_profile.py --case trained [--tables 1024] [--slice 16] [--reps 3]

A context of `--tables` f64 tables of 20^4 states (5.12 MB each), filled by

    --case trained     `--episodes` chained Philox training episodes of tables / 2 scenarios x 2 agents
                       at the bench's epsilon schedule (bench.epsilon_at): what a sweep checkpoints
    --case synthetic   the digest profile's tables: random normals, a third of the rows zero

Per repetition: get_q on a `--slice`-table range (q_unpack_kernel, the yardstick: the only export there was),
sparse_count over all tables, get_q_sparse over tables [0, export) (`--export`, default all of them: the
synthetic case exports 3 MB a table), set_q_sparse(zero=True) of the first half of that export over the
second half of the tables; then, after the repetitions, `--reps` times copy_q of table 0 over all the
others.  Prints one JSON line with the byte counts the per-byte times are formed from.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2pmicrogrid_amd.engine import DeviceCommunityBatch  # noqa: E402


def trained(tables, episodes, q_dtype):
    import bench
    from p2pmicrogrid_amd.dataset import scenario_batch
    S, N, T = tables // 2, 2, 96
    inp = scenario_batch(S, N, T)
    eng = DeviceCommunityBatch(S, N, 1, T, q_dtype=q_dtype)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    eng.run_episodes(0, [bench.epsilon_at(e) for e in range(episodes)], reset_sigma=0.3)
    eng.sync()
    return eng


def synthetic(tables, chunk_tables, q_dtype):
    eng = DeviceCommunityBatch(tables, 1, 0, 1, q_dtype=q_dtype)
    rs = np.random.RandomState(1)
    chunk = rs.standard_normal((chunk_tables, eng.n_states, 3))
    chunk[rs.rand(chunk_tables, eng.n_states) < 0.33] = 0.0
    for first in range(0, tables, chunk_tables):
        eng.set_q(chunk[:min(chunk_tables, tables - first)], first=first)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="trained", choices=["trained", "synthetic"])
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--slice", type=int, default=16)
    ap.add_argument("--export", type=int, default=0, help="tables get_q_sparse exports (0: all)")
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--q-dtype", default="f64")
    a = ap.parse_args()
    eng = trained(a.tables, a.episodes, a.q_dtype) if a.case == "trained" else synthetic(a.tables, a.slice, a.q_dtype)
    assert eng.n_tables == a.tables
    n_exp = a.export or a.tables
    half = min(n_exp, a.tables // 2)
    wall = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        out = fn()
        wall.setdefault(name, []).append(time.perf_counter() - t0)
        return out

    n_rows = eng.sparse_count()  # before the import below rewrites the second half
    for _ in range(a.reps):
        timed("get_q_slice", lambda: eng.get_q(0, a.slice))
        timed("sparse_count", eng.sparse_count)
        sp = timed("get_q_sparse", lambda: eng.get_q_sparse(0, n_exp))  # count, then count + offsets + scatter
        part = {"shape": sp["shape"], "offsets": sp["offsets"][:half + 1], "rows": sp["rows"][:sp["offsets"][half]],
                "values": sp["values"][:sp["offsets"][half]]}
        timed("set_q_sparse", lambda: eng.set_q_sparse(part, first=a.tables - half, zero=True))
    for _ in range(a.reps):
        timed("copy_q", lambda: eng.copy_q(0, 1, a.tables - 1))
    elem = 8 if a.q_dtype == "f64" else 4
    table_bytes = eng.n_states * 4 * elem
    row_bytes = 4 + 3 * elem
    stored = int(n_rows.sum())
    print(json.dumps({
        "case": a.case, "tables": a.tables, "slice": a.slice, "export_tables": n_exp, "import_tables": half,
        "q_dtype": a.q_dtype, "n_states": eng.n_states, "table_bytes": table_bytes,
        "bytes_read_all": table_bytes * a.tables, "bytes_read_slice": table_bytes * a.slice,
        "bytes_read_export": table_bytes * n_exp,
        "stored_rows_all": stored, "stored_fraction": stored / (a.tables * eng.n_states),
        "stored_rows_min_max": [int(n_rows.min()), int(n_rows.max())],
        "host_bytes": {"get_q_slice": a.slice * eng.n_states * 3 * elem, "sparse_count": 8 * a.tables,
                       "get_q_sparse": 8 * n_exp + row_bytes * int(sp["offsets"][-1]),
                       "set_q_sparse": 8 * half + row_bytes * int(sp["offsets"][half]), "copy_q": 0},
        "staging_runs_export_at_least": int(np.ceil(row_bytes * int(sp["offsets"][-1]) / (8 << 20))),
        "wall_s_min": {k: min(v) for k, v in wall.items()}}))


if __name__ == "__main__":
    main()
