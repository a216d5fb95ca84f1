"""Time the one-launch greedy DQN episode against the stepwise one at the same inputs.

    python scripts/dqn_eval_timing.py [--out times.json]

Per shape: HIP-event times (p2pmg_last_kernel_ms) of DeviceDQNBatch.run_greedy("online") (one launch of
dqn_greedy_episode_kernel) and of run_episode("greedy") (T act launches), warm, median of 11, both from
the same start temperatures and without records.  On a checkout from before run_greedy only the stepwise
form is timed.  Prints one JSON line per shape.  Networks: Glorot x 8 (the policy is not constant);
inputs: dataset.scenario_batch.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from p2pmicrogrid_amd.dataset import scenario_batch  # noqa: E402
from p2pmicrogrid_amd.dqn import DeviceDQNBatch, glorot_init  # noqa: E402

REPS, WARM = 11, 2
# label, S, N, R, T, one shared network
SHAPES = [("configs[4] shape, one shared network", 4096, 2, 1, 96, True),
          ("test days", 5, 2, 1, 96, False),
          ("4096 x 2 x 96, per-agent networks", 4096, 2, 1, 96, False),
          ("one year", 64, 2, 1, 35040, False),
          ("wide form", 256, 24, 1, 96, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write every row to this JSON file")
    args = ap.parse_args()
    rows = []
    for label, S, N, R, T, shared in SHAPES:
        t0 = time.time()
        inp = scenario_batch(S, N, T)
        eng = DeviceDQNBatch(S, N, R, T, shared=shared, capacity=32, init_seed=None)
        th = glorot_init(eng.n_nets, 0) * np.float32(8.0)
        eng.set_weights("online", th)
        eng.set_weights("target", th)
        eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
        eng.set_profiles(inp.load_w, inp.pv_w)
        eng.set_max_in(inp.max_in)
        row = {"label": label, "S": S, "N": N, "R": R, "T": T, "shared": shared}
        forms = (["one_launch"] if hasattr(eng, "run_greedy") else []) + ["stepwise"]
        for form in forms:
            ms, wall = [], []
            for _ in range(WARM + REPS):
                eng.set_temperatures(inp.t_in0, inp.t_m0)
                eng.sync()
                w0 = time.perf_counter()
                if form == "one_launch":
                    eng.run_greedy("online")
                else:
                    eng.run_episode("greedy")
                eng.sync()
                wall.append((time.perf_counter() - w0) * 1e3)
                ms.append(eng.last_kernel_ms())
            ms, wall = ms[WARM:], wall[WARM:]
            row[form] = {"kernel": eng.last_kernel(), "event_ms_median": float(np.median(ms)),
                         "event_ms_min": float(min(ms)), "event_ms_max": float(max(ms)),
                         "host_wall_ms_median": float(np.median(wall))}
        if "one_launch" in row:
            row["ratio_stepwise_over_one_launch"] = row["stepwise"]["event_ms_median"] / row["one_launch"]["event_ms_median"]
        row["setup_s"] = time.time() - t0
        eng.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
