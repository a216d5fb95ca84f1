"""Time the DQN role context (DeviceDQNBatch(shared="role")) against the forms it sits beside.

    python scripts/dqn_roles_timing.py [--forms per_agent,role,days] [--reps 9] [--out times.json]

Forms, one JSON line each:
  per_agent  HIP-event time (p2pmg_last_kernel_ms: the episode's T act + T train launches) of one Philox training
             episode at 4096 x 2 agents, T = 96, R = 1, per-agent networks, warm, `reps` episodes after two fill
             episodes (scripts/dqn_learning_timing.py's "default" form; runs on older checkouts too)
  role       the same episode on a role context: T act + T train + T reduce launches
  days       what train_days replaces: D = 64 days of one N = 2 community trained as 64 single-scenario episodes on
             one S = 1 engine (per day: env, profiles and temperatures uploaded, one training episode, sync), and as
             ONE training episode of a 64-scenario role engine (temperatures, episode, sync; its inputs uploaded
             once, timed apart).  Wall time of the Python calls, median of `reps`.
Inputs: dataset.scenario_batch; networks: Glorot.  Under `rocprofv3 --kernel-trace --stats` with one form, the
kernel statistics split an env step into its act, train and reduce launches.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from p2pmicrogrid_amd.dataset import scenario_batch  # noqa: E402
from p2pmicrogrid_amd.dqn import DeviceDQNBatch  # noqa: E402

S, N, R, T = 4096, 2, 1, 96
WARM = 2


def _engine(inp, shared, s=None):
    s = inp.max_in.shape[0] if s is None else s
    eng = DeviceDQNBatch(s, N, R, T, shared=shared, capacity=5000, init_seed=0)
    if s == inp.max_in.shape[0]:
        _upload(eng, inp, slice(None))
    return eng


def _upload(eng, inp, rows):
    eng.set_env(np.broadcast_to(inp.time, inp.t_out[rows].shape), inp.t_out[rows])
    eng.set_profiles(inp.load_w[rows], inp.pv_w[rows])
    eng.set_max_in(inp.max_in[rows])
    eng.set_temperatures(inp.t_in0[rows], inp.t_m0[rows])


def episode_events(shared, reps):
    inp = scenario_batch(S, N, T)
    eng = _engine(inp, shared)
    for ep in range(2):
        eng.run_episode("fill", "philox", episode=ep, epsilon=1.0)
    ms = []
    for k in range(WARM + reps):
        eng.run_episode("train", "philox", episode=2 + k, epsilon=0.5)
        eng.sync()
        ms.append(eng.last_kernel_ms())
    layout = eng.grad_layout() if shared else None
    kernel = eng.last_kernel()
    eng.close()
    ms = ms[WARM:]
    return {"S": S, "N": N, "T": T, "R": R, "kernel": kernel, "grad_layout": layout,
            "event_ms": [round(float(x), 4) for x in ms], "event_ms_median": float(np.median(ms)),
            "event_ms_min": float(min(ms)), "event_ms_max": float(max(ms)), "env_steps": T}


def days_wall(reps, D=64):
    inp = scenario_batch(D, N, T)
    one = _engine(inp, False, s=1)
    _upload(one, inp, slice(0, 1))
    t0 = time.perf_counter()
    role = _engine(inp, "role")
    role.sync()
    role_setup = time.perf_counter() - t0
    for eng in (one, role):
        for ep in range(2):
            eng.run_episode("fill", "philox", episode=ep, epsilon=1.0)
        eng.sync()
    by_day, at_once = [], []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        for d in range(D):
            _upload(one, inp, slice(d, d + 1))
            one.run_episode("train", "philox", episode=2 + k * D + d, epsilon=0.5)
            one.sync()
        by_day.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        role.set_temperatures(inp.t_in0, inp.t_m0)
        role.run_episode("train", "philox", episode=2 + k, epsilon=0.5)
        role.sync()
        at_once.append(time.perf_counter() - t0)
    one.close()
    role.close()
    by_day, at_once = by_day[WARM:], at_once[WARM:]
    return {"days": D, "N": N, "T": T, "R": R,
            "day_by_day_wall_ms": [round(1e3 * x, 3) for x in by_day], "day_by_day_wall_ms_median": 1e3 * float(np.median(by_day)),
            "role_episode_wall_ms": [round(1e3 * x, 3) for x in at_once], "role_episode_wall_ms_median": 1e3 * float(np.median(at_once)),
            "role_engine_setup_wall_ms": 1e3 * role_setup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default="per_agent,role,days")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write every row to this JSON file")
    args = ap.parse_args()
    rows = []
    for form in args.forms.split(","):
        if form == "per_agent":
            row = episode_events(False, args.reps)
        elif form == "role":
            row = episode_events("role", args.reps)
        elif form == "days":
            row = days_wall(args.reps)
        else:
            raise SystemExit(f"unknown form {form!r}")
        row = {"form": form, **row}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
