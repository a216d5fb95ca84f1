"""The input sets of the day-profile tests: the episode-summary cases (tests/summary_cases.py, as they are),
the argument variants, and the expected arrays (tests/day_profile_ref.py on the ORACLE's episode).  Each oracle episode is computed once per process."""
import functools

import numpy as np

import day_profile_ref
import summary_cases
from oracle.restatement import OracleParams

F32 = np.float32
# every kernel family, N in {1, 2, 3, 4, 5, 10, 16}, T = 1
CASES = ("fast_train", "general", "tile", "sq16_many", "shared_general_many", "role", "mixed", "battery", "rule",
         "dqn", "one_step", "one_agent")
VARIANT_CASES = ("sq16_many", "general")


@functools.lru_cache(maxsize=None)
def episode(name):
    """{"case", "inp", "out", "levels" [S, N, 3], "lower", "upper" [S, N], "reward" (recorded or not)}."""
    e = summary_cases.expected(name)
    c, inp, out = e["case"], e["inp"], e["out"]
    levels = c.hp_levels()
    if levels is None:
        levels = np.broadcast_to(OracleParams().hp_levels, (c.S, c.N, 3))
    lower, upper = c.bounds()
    return {"case": c, "inp": inp, "out": out, "levels": levels, "lower": lower, "upper": upper, "reward": c.kind != "rule"}


def want_from(e, out=None, reward=None, **kw):
    """The four expected arrays for the episode dict ``e`` (or for other records ``out`` of the same inputs)."""
    return day_profile_ref.profile(e["out"] if out is None else out, e["levels"], e["inp"].load_w, e["inp"].pv_w,
                                   e["lower"], e["upper"], reward=e["reward"] if reward is None else reward, **kw)


@functools.lru_cache(maxsize=None)
def want(name, variant="whole"):
    e = episode(name)
    kw = dict(variants(e["case"]))[variant]
    res = want_from(e, **kw)
    for a in res:
        a.setflags(write=False)
    return res


def variants(c):
    """[(tag, day_profile / helper keyword arguments)] for a case of S scenarios and T steps."""
    S, T = c.S, c.T
    mod3 = np.arange(S) % 3
    holes = np.array([0, 1, 3])[mod3]  # group 2 of 4 stays empty ...
    holes[1 % S] = -1                  # ... and one scenario is left out
    out = [("whole", {}), ("period_1", {"period": 1}), ("period_7", {"period": 7}), ("period_12", {"period": 12}),
           ("steps", {"steps": (5, T - 9)}), ("steps_folded", {"steps": (5, T - 9), "period": 7}),
           ("scenarios", {"scenarios": (1, S) if S < 4 else (3, S - 3)}),
           # neighbouring scenarios in different groups
           ("mod3", {"groups": mod3, "n_groups": 3}),
           ("mod3_folded", {"groups": mod3, "n_groups": 3, "period": 7, "steps": (2, T - 1)}),
           # the same labels sorted: runs of one group
           ("sorted", {"groups": np.sort(mod3), "n_groups": 3}),
           ("holes", {"groups": holes, "n_groups": 4}),
           ("holes_range", {"groups": holes, "n_groups": 4, "scenarios": (0, S - 1), "period": 12})]
    if T >= 96:
        out.append(("period_96", {"period": 96}))
    return out
