"""Wall time of DeviceCommunityBatch.day_profile() against the five get_record copies it replaces
(profiles/day_profile/README.md).  Per shape: one greedy launch with full records, then the median of
`calls` synchronising calls after 3 warm-up calls, each side on the same context:
  profile  day_profile() (whole, G = 1): init, agent, community and decode kernels + the four arrays to the host
  copies   get_record of cost, grid, p2p, t_in, action (P2PMG_SUMMARY_RECORDS): copies only, no host arithmetic
reported without a threshold: day_profile.from_records on the copied records (once), interleaved labels with
G = 3, the profile at each --tiles budget (P2PMG_DAYPROF_TILE_BYTES), and for `year` the fold period=96.
usage: probe_day_profile.py [--calls 20] [--shapes fast,sq16[,year]] [--tiles 8192,16384,32768,65536] [--host-form]
  fast  S = 4096,  N = 2,  T = 96     per-agent f64 tables, episode_fast_kernel (packed rows)
  sq16  S = 16384, N = 16, T = 96     one shared f32 table, episode_sq16_kernel (2^18 agents, packed rows)
  year  S = 512,   N = 4,  T = 35040  a one-year episode"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2pmicrogrid_amd import day_profile
from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.engine import SUMMARY_RECORDS, DeviceCommunityBatch
from probe_summary import SHAPES, median_ms

ENV = "P2PMG_DAYPROF_TILE_BYTES"


def stats(fn, calls):
    med, lo, hi = median_ms(fn, calls)
    return {"median": med, "min": lo, "max": hi}


def probe(name, calls, tiles, host_form):
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
    os.environ.pop(ENV, None)
    kw = {"period": 96} if name == "year" else {}
    line = {"shape": name, "S": S, "N": N, "T": T, "agents": S * N, "kernel": eng.last_kernel(), "calls": calls,
            "arguments": kw, "episode_kernel_ms": eng.last_kernel_ms(),
            "profile_ms": stats(lambda: eng.day_profile(**kw), calls),
            "copies_ms": stats(lambda: eng.get_records(SUMMARY_RECORDS), calls),
            "summary_ms": stats(eng.episode_summary, calls),
            "labels3_ms": stats(lambda: eng.day_profile(groups=np.arange(S) % 3, n_groups=3, **kw), calls),
            "profile_bytes_to_host": sum(a.nbytes for a in eng.day_profile(**kw)),
            "copies_bytes_to_host": T * S * N * (4 * 4 + (R + 1)), "tiles_ms": {}}
    line["profile_faster"] = line["profile_ms"]["median"] < line["copies_ms"]["median"]
    for tile in tiles:
        os.environ[ENV] = str(tile)
        line["tiles_ms"][str(tile)] = stats(lambda: eng.day_profile(**kw), calls)
    os.environ.pop(ENV, None)
    if host_form:
        rec = eng.get_records(("reward",) + SUMMARY_RECORDS)
        th = eng.get_thermal()
        t0 = time.perf_counter()
        want = day_profile.from_records(rec, eng.get_hp_levels(), inp.load_w, inp.pv_w, th[..., 1], th[..., 2], **kw)
        line["from_records_ms"] = (time.perf_counter() - t0) * 1e3
        line["equal_to_from_records"] = all(np.array_equal(a, b) for a, b in zip(eng.day_profile(**kw), want))
    eng.close()
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shapes", default="fast,sq16")
    ap.add_argument("--tiles", default="8192,16384,32768,65536")
    ap.add_argument("--host-form", action="store_true", help="also time day_profile.from_records on the copied records")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        print(json.dumps(probe(shape, a.calls, [int(t) for t in a.tiles.split(",") if t], a.host_form)), flush=True)
