"""Time a DQN train episode with per-agent networks: what the per-network constants cost the existing path.

    python scripts/dqn_learning_timing.py [--out times.json]

HIP-event time (p2pmg_last_kernel_ms: the episode's T act + T train launches) of
DeviceDQNBatch.run_episode("train", "philox") at 4096 x 2 agents, T = 96, per-agent networks, warm, median
of 9 after two fill episodes.  Runs on a checkout from before DeviceDQNBatch.set_learning too (the "default"
form alone), so the same command on both trees gives the comparison.  Forms:
  default   no set_learning call: every network's constants equal, the scalar kernel arguments
  mixed     every network its own (gamma, tau, lr, clip): the train kernel loads its row, the episode
            uploads a [T][n_nets] step-size table
Prints one JSON line per form.  Inputs: dataset.scenario_batch; networks: Glorot.
"""
import argparse
import inspect
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from p2pmicrogrid_amd.dataset import scenario_batch  # noqa: E402
from p2pmicrogrid_amd.dqn import DeviceDQNBatch  # noqa: E402

S, N, R, T = 4096, 2, 1, 96
REPS, WARM = 9, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write every row to this JSON file")
    args = ap.parse_args()
    inp = scenario_batch(S, N, T)
    rows = []
    eng = DeviceDQNBatch(S, N, R, T, shared=False, capacity=5000, init_seed=0)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    for ep in range(2):
        eng.run_episode("fill", "philox", episode=ep, epsilon=1.0)
    episode = 2
    for form in ["default"] + (["mixed"] if "tau" in inspect.signature(DeviceDQNBatch.set_learning).parameters else []):
        if form == "mixed":
            u = np.random.RandomState(0).uniform(size=(4, S, N))
            eng.set_learning(gamma=0.9 + 0.1 * u[0], tau=0.001 + 0.05 * u[1], lr=1e-5 * (1 + u[2]), clip=0.5 + u[3])
        ms = []
        for _ in range(WARM + REPS):
            eng.run_episode("train", "philox", episode=episode, epsilon=0.5)
            eng.sync()
            ms.append(eng.last_kernel_ms())
            episode += 1
        ms = ms[WARM:]
        row = {"form": form, "S": S, "N": N, "T": T, "event_ms": [round(float(x), 4) for x in ms],
               "event_ms_median": float(np.median(ms)), "event_ms_min": float(min(ms)), "event_ms_max": float(max(ms))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
