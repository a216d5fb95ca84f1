"""Drive the table digests and get_q's device pass over the same tables, for a kernel trace
(profiles/table_digest/README.md):

    rocprofv3 --kernel-trace --stats -d <dir> -o td --output-format csv -- \\
        python scripts/table_digest_profile.py [--tables 1024] [--slice 16] [--reps 3]

A context of `--tables` f64 tables of 20^4 states (5.12 MB each); get_q on a `--slice`-table range
(q_unpack_kernel, the yardstick: it reads the same padded rows and writes 3/4 as much), then table_stats,
greedy_policy, policy_mark and policy_changes(remark=True) over all tables, `--reps` times each.
Prints one JSON line with the byte counts the per-byte times are formed from.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2pmicrogrid_amd.engine import DeviceCommunityBatch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--slice", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--q-dtype", default="f64")
    a = ap.parse_args()
    eng = DeviceCommunityBatch(a.tables, 1, 0, 1, q_dtype=a.q_dtype)
    rs = np.random.RandomState(1)
    chunk = rs.standard_normal((a.slice, eng.n_states, 3))
    chunk[rs.rand(a.slice, eng.n_states) < 0.33] = 0.0
    for first in range(0, a.tables, a.slice):
        eng.set_q(chunk[:min(a.slice, a.tables - first)], first=first)
    wall = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        out = fn()
        wall.setdefault(name, []).append(time.perf_counter() - t0)
        return out

    eng.policy_mark()
    for _ in range(a.reps):
        timed("get_q_slice", lambda: eng.get_q(0, a.slice))
        st = timed("table_stats", eng.table_stats)
        timed("greedy_policy", eng.greedy_policy)
        timed("policy_mark", eng.policy_mark)
        ch = timed("policy_changes_remark", lambda: eng.policy_changes(remark=True))
    elem = 8 if a.q_dtype == "f64" else 4
    table_bytes = eng.n_states * 4 * elem
    print(json.dumps({"tables": a.tables, "slice": a.slice, "q_dtype": a.q_dtype, "n_states": eng.n_states,
                      "table_bytes": table_bytes, "bytes_read_all": table_bytes * a.tables,
                      "bytes_read_slice": table_bytes * a.slice, "visited_0": int(st["visited"][0]),
                      "changed_sum": int(ch["changed"].sum()),
                      "wall_s_min": {k: min(v) for k, v in wall.items()}}))


if __name__ == "__main__":
    main()
