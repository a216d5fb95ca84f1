"""DQN evaluation without a GPU: the three calls exist, are bound and refuse a NULL context; the default
agent -> network map as a pure function; and the seeds and scales of the GPU tests' cases give a policy
that is not constant on the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import dqn_eval_cases as dc
from p2pmicrogrid_amd import _build, _lib
from p2pmicrogrid_amd.dqn import default_net_map

NEW = ("p2pmg_dqn_set_policy_nets", "p2pmg_dqn_get_policy_nets", "p2pmg_dqn_run_greedy")
E_INVALID = 1


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int, name
    assert _lib.DQN_POLICY_SET == 4 and _lib.DQN_POLICY_SET not in (_lib.DQN_ONLINE, _lib.DQN_TARGET, _lib.DQN_ADAM_M,
                                                                    _lib.DQN_ADAM_V)
    header = open(os.path.join(_build.ROOT, "include", "p2pmg.h")).read()
    assert "#define P2PMG_DQN_POLICY_SET 4" in header
    bump = next(line for line in header.splitlines() if line.startswith("#define P2PMG_ABI_VERSION"))
    assert all(name in bump.split("added since without a bump")[1] for name in NEW + ("P2PMG_DQN_POLICY_SET",))
    assert ("p2pmg_dqn_eval.hip", None, [], "p2pmg_dqn_eval.o") in _build.UNITS


def test_null_context_is_invalid():
    L = _lib.lib()
    n = C.c_int(7)
    w = np.zeros((1, _lib.DQN_PARAMS), np.float32)
    assert L.p2pmg_dqn_set_policy_nets(None, 1, w.ctypes.data, None) == E_INVALID
    assert L.p2pmg_dqn_get_policy_nets(None, C.byref(n), None, None) == E_INVALID
    assert L.p2pmg_dqn_run_greedy(None, _lib.DQN_ONLINE, 0) == E_INVALID
    assert L.p2pmg_dqn_run_greedy(None, _lib.DQN_POLICY_SET, 0) == E_INVALID


@pytest.mark.parametrize("count,S,N,want", dc.default_map_cases())
def test_default_map_rule(count, S, N, want):
    """a % count for count == N, the identity for count == A, all 0 for count == 1; anything else raises."""
    if want is None:
        with pytest.raises(ValueError):
            default_net_map(count, S, N)
        return
    got = default_net_map(count, S, N)
    assert got.dtype == np.int32 and got.shape == (S * N,) and np.array_equal(got, want)


@pytest.mark.parametrize("name", list(dc.CASES))
def test_case_policies_are_not_constant(name):
    c = dc.CASES[name]
    act = dc.oracle_actions(c, dc.case_weights(c))
    assert act.shape == (c.T, c.R + 1, c.S, c.N)
    assert len(np.unique(act)) >= dc.actions_needed(c), np.bincount(act.ravel(), minlength=3)


def test_policy_set_cases_are_not_constant():
    c = dc.ROLE
    assert len(np.unique(dc.oracle_actions(c, dc.tiled(dc.weights(c.N, c.seed, c.scale), c.S)))) == 3
    c = dc.ARBITRARY
    nets = dc.weights(2, c.seed, c.scale)
    assert len(np.unique(dc.oracle_actions(c, nets[dc.ARBITRARY_MAP]))) == 3
    assert not np.array_equal(nets[0], nets[1]) and sorted(set(dc.ARBITRARY_MAP)) == [0, 1]
    c = dc.CASES["s3n2r1t12"]  # the target network of the source="target" test
    assert len(np.unique(dc.oracle_actions(c, dc.weights(c.S * c.N, c.seed + 50, c.scale)))) == 3
