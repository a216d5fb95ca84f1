"""Wall time of DeviceCommunityBatch.episode_summary() against the five get_record copies it
replaces (profiles/summary/README.md).  Per shape: one greedy launch with full records, then the
median of `calls` synchronising calls after 3 warm-up calls, each side on the same context:
  summary  episode_summary(): two kernels + [A][16] and [S][16] f64 copied to the host
  copies   get_record of cost, grid, p2p, t_in, action (P2PMG_SUMMARY_RECORDS): copies only, no host sums
usage: probe_summary.py [--calls 20] [--shapes fast,sq16[,year]]   (one JSON line per shape)
  fast  S = 4096,  N = 2,  T = 96     per-agent f64 tables, episode_fast_kernel (packed rows)
  sq16  S = 16384, N = 16, T = 96     one shared f32 table, episode_sq16_kernel (2^18 agents, packed rows)
  year  S = 512,   N = 4,  T = 35040  a one-year episode: one long sequential loop per lane"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.engine import SUMMARY_RECORDS, DeviceCommunityBatch

SHAPES = {"fast": (4096, 2, 1, 96, "f64", False), "sq16": (16384, 16, 1, 96, "f32", True),
          "year": (512, 4, 1, 35040, "f64", False)}


def median_ms(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()  # ends in a stream synchronise
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def probe(name, calls):
    S, N, R, T, q_dtype, shared = SHAPES[name]
    inp = scenario_batch(S, N, T, seed=7)
    eng = DeviceCommunityBatch(S, N, R, T, q_dtype=q_dtype, shared_q=shared)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    if shared:
        eng.set_q(np.random.RandomState(5).standard_normal((1, 20 ** 4, 3)).astype(np.float32))
    eng.run_episode("greedy", record=("reward",) + SUMMARY_RECORDS)
    eng.sync()
    s_med, s_min, s_max = median_ms(eng.episode_summary, calls)
    c_med, c_min, c_max = median_ms(lambda: eng.get_records(SUMMARY_RECORDS), calls)
    line = {"shape": name, "S": S, "N": N, "T": T, "agents": S * N, "kernel": eng.last_kernel(), "calls": calls,
            "episode_kernel_ms": eng.last_kernel_ms(),
            "summary_ms": {"median": s_med, "min": s_min, "max": s_max},
            "copies_ms": {"median": c_med, "min": c_min, "max": c_max},
            "summary_bytes_to_host": (S * N + S) * 16 * 8, "copies_bytes_to_host": T * S * N * (4 * 4 + (R + 1)),
            "summary_faster": s_med < c_med}
    eng.close()
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shapes", default="fast,sq16")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        print(json.dumps(probe(shape, a.calls)), flush=True)
