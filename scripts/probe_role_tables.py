"""One kernel-trace workload for profiles/role_tables/: N = 2, R = 1, T = 96, f64, S = 4096 on the
general episode kernel, per-role tables ("role") or one shared table ("shared"); 12 launches.
usage: probe_role_tables.py role|shared greedy|train   (P2PMG_LIB selects another build's library)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p2pmicrogrid_amd.dataset import scenario_batch
from p2pmicrogrid_amd.engine import DeviceCommunityBatch

mode, phase = sys.argv[1], sys.argv[2]
S, N, R, T = 4096, 2, 1, 96
inp = scenario_batch(S, N, T, seed=7)
eng = DeviceCommunityBatch(S, N, R, T, shared_q="role" if mode == "role" else True)
eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
eng.set_profiles(inp.load_w, inp.pv_w)
eng.set_max_in(inp.max_in)
eng.set_temperatures(inp.t_in0, inp.t_m0)
n_tab = N if mode == "role" else 1
eng.set_q(np.random.RandomState(5).standard_normal((n_tab, 20 ** 4, 3)))
for e in range(12):  # 2 warm-up + 10
    if phase == "greedy":
        eng.run_episode("greedy", kernel="general")
    else:
        eng.run_episode("train", "philox", episode=e, epsilon=0.3, kernel="general")
        eng.apply_q_delta()
eng.sync()
ms = eng.kernel_times()
print(mode, phase, eng.last_kernel(), "event ms, last 10: median %.4f min %.4f max %.4f" %
      (np.median(ms[2:]), ms[2:].min(), ms[2:].max()))
eng.close()
