"""The per-role-table expectations (tests/role_tables.py) against the oracle's own shared table: at
N = 1 one table per role IS one table for all, so the helper's deltas must equal
OracleBatch(shared_q=True).q_delta exactly.  Plus what of role mode can be checked without a GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle.restatement import OracleBatch, reference_replay_codes
from p2pmicrogrid_amd.dataset import scenario_batch
from role_tables import applied, frozen_oracle, random_tables, role_deltas


@pytest.mark.parametrize("R", [0, 1])
@pytest.mark.parametrize("q_dtype", ["f64", "f32"])
def test_delta_helper_equals_shared_oracle_at_one_agent(R, q_dtype):
    S, N, T, eps = 6, 1, 12, 0.5
    inp = scenario_batch(S, N, T, seed=3)
    tables = random_tables(N, q_dtype)
    rss = [np.random.RandomState(11 + s) for s in range(S)]
    codes = np.stack([reference_replay_codes(rs, T, R, N, eps) for rs in rss], axis=2)
    shared = OracleBatch(S=S, N=N, R=R, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in,
                         env_time=inp.time[None], env_tout=inp.t_out, q_dtype=q_dtype, shared_q=True)
    shared.q[0] = tables[0]
    shared.t_in, shared.t_m = inp.t_in0.copy(), inp.t_m0.copy()
    want = shared.run_episode("train", codes=codes, eps=eps)
    assert np.count_nonzero(shared.q_delta) > S  # the episode did learn something

    frozen = frozen_oracle(inp, N, R, tables, q_dtype)
    out = frozen.run_episode("train", codes=codes, eps=eps)
    assert np.array_equal(frozen.q, np.tile(tables, (S, 1, 1)))  # alpha = 0 froze the tables
    for k in ("action", "idx", "reward", "cost", "t_in"):
        assert np.array_equal(out[k], want[k]), k
    delta = role_deltas(frozen, out, tables)
    assert delta.shape == (1, 20 ** 4, 3) and np.array_equal(delta[0], shared.q_delta)
    shared.apply_q_delta()
    assert np.array_equal(applied(tables, delta)[0], shared.q[0])


def test_create_refuses_role_tables_with_dqn():
    """shared_q = P2PMG_SHARED_ROLE with the DQN learner: UNSUPPORTED before any device call, with
    the reason in p2pmg_last_error(NULL)."""
    from p2pmicrogrid_amd import _lib
    L = _lib.lib()
    cfg = _lib.default_config()
    cfg.shared_q, cfg.learner = _lib.SHARED_ROLE, _lib.LEARNER_DQN
    ctx = C.c_void_p()
    assert L.p2pmg_create(C.byref(cfg), 0, C.byref(ctx)) == 5 and not ctx.value
    assert b"P2PMG_SHARED_ROLE" in L.p2pmg_last_error(None)
    cfg.n_agents = 0  # a later failure that gives no reason clears it
    assert L.p2pmg_create(C.byref(cfg), 0, C.byref(ctx)) == 1
    assert L.p2pmg_last_error(None) == b"null context"


def test_python_layers_accept_only_the_three_modes():
    from p2pmicrogrid_amd.distributed import ShardedTrainer
    from p2pmicrogrid_amd.engine import DeviceCommunityBatch
    with pytest.raises(ValueError):
        DeviceCommunityBatch(1, 2, 1, 12, shared_q="roles")
    with pytest.raises(ValueError):
        ShardedTrainer(4, learner="dqn", shared_q="role")
    seen = {}

    def factory(sh, S, N, R, T, q_dtype, device, seed, shared_q=False):
        from oracle_engine import OracleEngine
        seen["shared_q"] = shared_q
        return OracleEngine(sh, S, N, R, T, q_dtype, device, seed, shared_q=False)
    tr = ShardedTrainer(2, 2, 0, 12, engine_factory=factory, shared_q="role")
    assert seen["shared_q"] == "role" and tr.shared_q == "role"
