"""The DQN policy map, host side: the new symbols, the default grid's bins, the reference's tie rule and
the Python wrappers' argument checks (no device)."""
import numpy as np
import pytest

import dqn_map_ref as ref
from oracle import restatement
from p2pmicrogrid_amd import _lib
from p2pmicrogrid_amd.dqn import DeviceDQNBatch

F32 = np.float32


def test_symbols_and_abi_version():
    assert _lib.ABI_VERSION == 9
    L = _lib.lib()
    assert L.p2pmg_abi_version() == 9
    for name in ("p2pmg_dqn_set_grid", "p2pmg_dqn_get_grid", "p2pmg_dqn_policy_map", "p2pmg_dqn_map_stats",
                 "p2pmg_dqn_policy_mark", "p2pmg_dqn_policy_changes"):
        assert hasattr(L, name), name
    assert _lib.DQN_MAP_STATS == 8


@pytest.mark.parametrize("shape", [(20, 20, 20, 20), (3, 4, 5, 7), (30, 20, 20, 30)])
def test_default_axes_are_their_own_bins(shape):
    """state_index of each default axis's centre k is k: a DQN map state and a table row are one bin."""
    axes = ref.default_axes(shape)
    for ax, K, kind in zip(axes, shape, ("time", "temp", "plain", "plain")):
        assert ax.dtype == F32 and ax.shape == (K,)
        assert np.array_equal(restatement.state_index(ax, K, kind), np.arange(K)), (kind, K)


def test_grid_order_is_time_slowest():
    axes = (np.array([1, 2], F32), np.array([10, 20, 30], F32), np.array([100], F32), np.array([7, 8], F32))
    obs = ref.grid_obs(axes)
    assert obs.shape == (12, 4)
    g = ((1 * 3 + 2) * 1 + 0) * 2 + 1
    assert np.array_equal(obs[g], np.array([2, 30, 100, 8], F32))
    assert np.array_equal(obs[1], np.array([1, 10, 100, 8], F32))


def test_argmax_takes_the_first_maximum():
    q = np.array([[1, 1, 1], [0, 2, 2], [3, 1, 3], [-1, -1, -0.5], [0.0, -0.0, 0.0]], F32)
    assert np.array_equal(ref.argmax_first(q), np.array([0, 1, 0, 2, 0], np.uint8))
    st = ref.fold_stats(q[:1], ref.argmax_first(q[:1]))
    assert st["min_gap"] == 0.0 and not np.signbit(st["min_gap"])
    assert list(st["greedy"]) == [1, 0, 0]


def test_map_ref_on_a_hand_made_tie():
    """W1[4, :] = 0 makes the three action rows identical: all three Q equal, the greedy action is 0."""
    from oracle import dqn as odqn
    th = odqn.glorot_init(1, seed=2)[0]
    th[4 * 64:5 * 64] = 0
    pol, q, st = ref.map_ref(th, ref.default_axes((3, 3, 2, 2)))
    assert np.array_equal(q[..., 0], q[..., 1]) and np.array_equal(q[..., 0], q[..., 2])
    assert not pol.any() and st["min_gap"] == 0.0 and list(st["greedy"]) == [36, 0, 0]


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the arguments were checked")


def _unbound(n_nets=3):
    eng = DeviceDQNBatch.__new__(DeviceDQNBatch)
    eng.n_nets, eng.L, eng._ctx = n_nets, _NoDevice(), None
    return eng


def test_wrappers_check_arguments_before_any_device_call():
    eng = _unbound()
    calls = (eng.policy_map, eng.map_stats, eng.map_changes)
    for f in calls:
        with pytest.raises(ValueError, match="which"):
            f(which="adam_m")
        for first, count in ((-1, 1), (0, 4), (3, 1), (1, -1), (2, 2)):
            with pytest.raises(ValueError, match="networks"):
                f(first=first, count=count)
    with pytest.raises(ValueError, match="which"):
        eng.map_mark(which="both")
    one = np.zeros(1, F32)
    with pytest.raises(ValueError, match="at least one"):
        eng.set_policy_grid(one, np.zeros(0, F32), one, one)
    with pytest.raises(ValueError, match="all four"):
        eng.set_policy_grid(one, None, one, one)
    with pytest.raises(ValueError, match="2\\^31"):
        big = np.zeros(1 << 11, F32)
        eng.set_policy_grid(big, big, big[:512], one)
