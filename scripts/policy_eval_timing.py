"""Time p2pmg_run_policy against the greedy launches it sits beside (profiles/policy_eval/README.md).

    python scripts/policy_eval_timing.py FORM [launches]

One form per process, one JSON line: HIP-event kernel time (p2pmg_last_kernel_ms) of `launches` warm launches
after 3 discarded ones, temperatures re-uploaded before each.  configs[1]'s shape, 4096 x 2, T = 96, R = 1,
records reward + cost, f64 per-agent tables written by three Philox training episodes:
  policy    run_policy with M == A policies captured from the tables
  rolemap   run_policy with M == N == 2 policies (the role map)
  general   run_episode("greedy", kernel="general")
  fast      run_episode("greedy"): the fast kernel
  capture   capture_policies() of the 8192 f64 tables against greedy_policy()'s host copy of the same bytes
            (wall time around a synchronised call, ms)
  capacity  2^20 agents (524288 x 2) with M == N random policies on a shared_q=True context
Run the forms alternating, each in its own process.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.engine import DeviceCommunityBatch

form = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 15
S, N, R, T = 4096, 2, 1, 96
REC = ("reward", "cost")

def setup(eng, inp):
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(inp.t_in0, inp.t_m0)

def timed(eng, inp, launch):
    ms = []
    for k in range(n + 3):
        eng.set_temperatures(inp.t_in0, inp.t_m0)
        launch()
        ms.append(eng.last_kernel_ms())
    return ms[3:]

out = {"form": form}
if form in ("policy", "general", "fast", "rolemap", "capture"):
    inp = scenario_batch(S, N, T)
    eng = DeviceCommunityBatch(S, N, R, T, alpha=0.3)
    setup(eng, inp)
    eng.run_episodes(0, [0.8, 0.6, 0.4], reset_sigma=0.3)   # tables with written rows
    if form == "policy":
        eng.set_policy_set(count=eng.A); eng.capture_policies()
        ms = timed(eng, inp, lambda: eng.run_policy(record=REC))
    elif form == "rolemap":
        eng.set_policy_set(count=N); eng.capture_policies(0, N, 0)
        ms = timed(eng, inp, lambda: eng.run_policy(record=REC))
    elif form == "general":
        ms = timed(eng, inp, lambda: eng.run_episode("greedy", record=REC, kernel="general"))
    elif form == "fast":
        ms = timed(eng, inp, lambda: eng.run_episode("greedy", record=REC))
    else:
        eng.set_policy_set(count=eng.A)
        cap, host = [], []
        for k in range(4):
            eng.sync(); t0 = time.perf_counter(); eng.capture_policies(); eng.sync(); cap.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); g = eng.greedy_policy(); host.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(eng.policy_set()[0], g)
        out.update(capture_ms=cap, greedy_policy_host_ms=host, tables=eng.n_tables)
        ms = []
    out["kernel"] = eng.last_kernel()
elif form == "capacity":
    S2 = 1 << 19  # 2^20 agents at N = 2, M = N policies
    base = scenario_batch(4096, N, T)
    rep = S2 // 4096
    class I: pass
    inp = I()
    inp.time = base.time
    for k in ("t_out", "load_w", "pv_w", "max_in", "t_in0", "t_m0"):
        setattr(inp, k, np.tile(getattr(base, k), (rep,) + (1,) * (getattr(base, k).ndim - 1)))
    eng = DeviceCommunityBatch(S2, N, R, T, shared_q=True, q_dtype="f32")
    setup(eng, inp)
    rs = np.random.RandomState(0)
    eng.set_policy_set(np.array([0, 1, 2, 255], np.uint8)[rs.randint(0, 4, (N, 160000))])
    ms = timed(eng, inp, lambda: eng.run_policy(record=REC))
    out.update(agents=S2 * N, kernel=eng.last_kernel())
    S = S2
if ms:
    med = float(np.median(ms))
    out.update(ms=[round(x, 4) for x in ms], median_ms=med, min_ms=min(ms), max_ms=max(ms),
               agent_steps_per_s=S * N * T / (med * 1e-3))
print(json.dumps(out), flush=True)
eng.close()
