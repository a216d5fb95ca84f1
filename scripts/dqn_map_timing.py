"""Time the DQN policy map against the only way to get the same bytes without it.

    python scripts/dqn_map_timing.py --mode map      --shape per_agent|shared|configs4
    python scripts/dqn_map_timing.py --mode baseline --shape per_agent|shared

map       DeviceDQNBatch.policy_map() (one byte per state to the host) and map_stats() (eight numbers per
          network: the pass alone) on the default 20^4 grid.
baseline  a loop over the networks of DeviceDQNBatch.q_values() on the same grid's observations with the
          argmax in NumPy: it needs nothing of the map, so it also runs on a checkout from before it.
Shapes: per_agent = 64 networks (S = 32, N = 2), shared = one network, configs4 = the 8,192 per-agent
networks of BASELINE.json configs[4] (map only).  One process per run; prints one JSON line.  The f32 MFMA
fraction counts layer 2 only (rows x 64 x 64 x 2 FLOP) against the 157.3 TF peak of the rooflines in DESIGN.md.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.environ.get("P2PMG_TIMING_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from p2pmicrogrid_amd.dqn import DeviceDQNBatch, glorot_init  # noqa: E402

F32 = np.float32
PEAK_F32_MFMA = 157.3e12
SHAPES = {"per_agent": (32, 2, False), "shared": (1, 1, True), "configs4": (4096, 2, False)}


def default_obs(K=20):
    k = np.arange(K, dtype=np.float64)
    ax = [((k + 0.5) / K).astype(F32), (2.0 * (k - 0.5) / (K - 2) - 1.0).astype(F32),
          (2.0 * (k + 0.5) / K - 1.0).astype(F32), (2.0 * (k + 0.5) / K - 1.0).astype(F32)]
    return np.stack([m.reshape(-1) for m in np.meshgrid(*ax, indexing="ij")], axis=-1).astype(F32)


def baseline_policy(eng, obs, nets):
    return np.stack([np.argmax(eng.q_values(obs, net), axis=1).astype(np.uint8) for net in nets])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["map", "baseline"], required=True)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="per_agent")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    S, N, shared = SHAPES[args.shape]
    eng = DeviceDQNBatch(S, N, 0, 1, shared=shared, init_seed=None, capacity=32)
    nn = eng.n_nets
    eng.set_weights("online", glorot_init(nn, 7))
    obs = default_obs()
    G = len(obs)
    out = {"mode": args.mode, "shape": args.shape, "networks": nn, "states": G, "reps": args.reps}
    if args.mode == "baseline":
        baseline_policy(eng, obs, [0])  # warm-up
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            pol = baseline_policy(eng, obs, range(nn))
            ts.append(time.perf_counter() - t0)
        out.update(policy_s=min(ts), policy_s_all=ts, checksum=int(pol.sum(dtype=np.int64)))
    else:
        eng.map_stats(0, 1)  # warm-up: the default grid, the first launch
        tp, tst = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            pol = eng.policy_map()
            tp.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            st = eng.map_stats()
            tst.append(time.perf_counter() - t0)
        same = bool(np.array_equal(pol[nn - 1].reshape(-1), baseline_policy(eng, obs, [nn - 1])[0]))
        flop = float(nn) * G * 3 * 64 * 64 * 2
        out.update(policy_s=min(tp), policy_s_all=tp, stats_s=min(tst), stats_s_all=tst,
                   checksum=int(pol.sum(dtype=np.int64)), same_bytes_as_q_values=same,
                   greedy=[int(x) for x in st["greedy"].sum(axis=0)],
                   mfma_tflops=flop / min(tst) / 1e12, mfma_fraction_of_peak=flop / min(tst) / PEAK_F32_MFMA)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
