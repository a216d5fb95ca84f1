"""The object API with heat pumps, COPs and setpoints that differ per agent: CommunityMicrogrid
uploads every agent's own values (community.thermal_arrays) for tabular, rule and DQN communities,
and HPHeating.step / temperature_simulation honour the COP and the solar term.

The communities are built with the constructors, homogeneous (T0 = setpoint, no T0 draws between
the replayed exploration draws), and checked against the oracle fed the community's own inputs."""
import numpy as np
import pytest

from oracle.restatement import OracleBatch, OracleParams, reference_replay_codes, temperature_step

pytestmark = pytest.mark.gpu
F32 = np.float32
PUMPS = ((3.0, 5e3), (4.0, 3e3), (2.5, 2e3))  # (cop, max_power)
SETPOINTS = (22.0, 21.0, 19.5)


def _community(kind, pumps, setpoints, R, T, seed=17):
    """(community, inputs): N agents of one kind over scenario_batch inputs."""
    from p2pmicrogrid_amd.agent import Agent, DQNAgent, QAgent, RuleAgent
    from p2pmicrogrid_amd.community import CommunityMicrogrid
    from p2pmicrogrid_amd.dataset import ProfileDataset, scenario_batch
    from p2pmicrogrid_amd.environment import env
    from p2pmicrogrid_amd.heating import HeatPump, HPHeating
    from p2pmicrogrid_amd.production import PV, Prosumer
    from p2pmicrogrid_amd.storage import NoStorage
    N = len(pumps)
    inp = scenario_batch(1, N, T, seed=seed)
    ds = lambda x: ProfileDataset(np.asarray(x, F32), np.roll(np.asarray(x, F32), -1, 0))  # noqa: E731
    ctor = {"q": QAgent, "rule": RuleAgent, "dqn": DQNAgent}[kind]
    Agent.reset_ids()
    agents = [ctor(ds(inp.load_w[0, i]), Prosumer(PV(float(inp.pv_ratings[0, i]) * 1e3, ds(inp.pv_w[0, i]))),
                   NoStorage(), HPHeating(HeatPump(cop, mp, 0.0), sp), max_in=float(inp.max_in[0, i]),
                   max_out=-float(inp.max_in[0, i]))
              for i, ((cop, mp), sp) in enumerate(zip(pumps, setpoints))]
    env.setup(ds(np.stack([inp.time, inp.t_out[0]], axis=1)))
    return CommunityMicrogrid(list(range(T)), agents, R)


def _oracle(com, R, T):
    """The oracle on the community's own inputs and the agents' own thermal parameters."""
    from p2pmicrogrid_amd.environment import env
    agents = com.agents
    N = len(agents)
    time_f, t_out = env.arrays()
    sp = np.array([[a.heating._temperature_setpoint for a in agents]])
    cop = np.array([[a.heating.hp.cop for a in agents]])
    lv = np.array([[[F32(l * a.heating.hp.max_power) for l in (0.0, 0.5, 1.0)] for a in agents]], F32)
    ob = OracleBatch(S=1, N=N, R=R, load_w=np.stack([a.load_series(T) for a in agents])[None],
                     pv_w=np.stack([a.pv.series(T) for a in agents])[None],
                     max_in=np.array([[F32(a.max_in) for a in agents]], F32), env_time=time_f[None],
                     env_tout=t_out[None], params=OracleParams(setpoint=sp, hp_cop=cop), hp_levels=lv)
    ob.t_in = np.array([[a.heating.temperature[0] for a in agents]], F32)
    ob.t_m = np.array([[a.heating.building_mass_temperature[0] for a in agents]], F32)
    return ob


def _homogeneous():
    from p2pmicrogrid_amd import setup

    class Flag:
        def __enter__(self):
            self.was = setup.homogeneous
            setup.homogeneous = True

        def __exit__(self, *exc):
            setup.homogeneous = self.was
    return Flag()


def _train_and_check(com, ob, rs, R, T, tag):
    N = len(com.agents)
    eps = float(com.agents[0].actor._epsilon)
    codes = reference_replay_codes(rs, T, R, N, eps)  # the draws train_episode takes from np.random
    reward, loss = com.train_episode()
    out = ob.run_episode("train", codes=codes[:, :, None, :], eps=eps)
    assert loss == 0.0
    assert np.array_equal(com.last_rewards, out["reward"][:, 0]), tag
    assert reward == float(out["episode_reward"][0]), tag
    mp = np.array([a.heating.hp.max_power for a in com.agents])
    assert np.array_equal(com.decisions, np.array([0.0, 0.5, 1.0])[out["action"][:, :, 0]] * mp), tag
    assert np.array_equal(np.stack([a.actor.q_table.reshape(-1, 3) for a in com.agents]), ob.q), tag
    # homogeneous reset: T0 = each agent's own setpoint
    ob.t_in = np.array([[a.heating.temperature[0] for a in com.agents]], F32)
    ob.t_m = np.array([[a.heating.building_mass_temperature[0] for a in com.agents]], F32)


def _run_and_check(com, ob, tag):
    power, cost = com.run()
    out = ob.run_episode("greedy")
    assert np.array_equal(power, (out["grid"][:, 0] + out["p2p"][:, 0]).astype(F32)), tag
    assert np.array_equal(cost, out["cost"][:, 0]), tag


@pytest.mark.parametrize("pumps,setpoints", [(PUMPS, SETPOINTS), (((3.0, 5e3),) * 3, (22.0,) * 3)],
                         ids=["mixed", "uniform-5kW"])
def test_tabular_community_uses_each_agents_pump_and_setpoint(pumps, setpoints):
    R, T = 1, 24
    with _homogeneous():
        com = _community("q", pumps, setpoints, R, T)
        ob = _oracle(com, R, T)
        np.random.seed(42)  # train_episode replays its exploration from the global np.random
        rs = np.random.RandomState(42)
        for e in range(2):
            _train_and_check(com, ob, rs, R, T, e)
        _run_and_check(com, ob, "run")
        if pumps is PUMPS:
            # another pump size between calls: uploaded again, decisions and simulation follow
            com.agents[0].heating.hp.max_power = 3e3
            q = ob.q
            ob = _oracle(com, R, T)
            ob.q = q
            _train_and_check(com, ob, rs, R, T, "re-upload")
        com._engine.close()


def test_rule_community_uses_each_agents_thresholds():
    T = 48
    with _homogeneous():
        com = _community("rule", PUMPS, SETPOINTS, 0, T)
        for a, sp in zip(com.agents, SETPOINTS):
            a.heating.set_state(sp - 1.2, sp - 1.2)
        ob = _oracle(com, 0, T)
        power, cost = com.run()
        out = ob.run_rule_episode(np.zeros((1, len(PUMPS)), F32))
        assert np.array_equal(power, (out["grid"][:, 0] + out["p2p"][:, 0]).astype(F32))
        assert np.array_equal(cost, out["cost"][:, 0])
        assert np.array_equal(com.decisions[:, 0, :], out["hp"][:, 0].astype(np.float64))
        assert [a.heating.hp.power for a in com.agents] == [float(x) for x in out["hp_on"][0]]
        assert out["on"].any() and not out["on"].all()
        com._engine.close()


def test_dqn_community_uploads_each_agents_values():
    from p2pmicrogrid_amd.community import thermal_arrays
    import random
    with _homogeneous():
        com = _community("dqn", PUMPS, SETPOINTS, 1, 8)
        np.random.seed(42)
        random.seed(42)
        com.init_buffers()
        levels, params = thermal_arrays(com.agents)
        assert np.array_equal(com._engine.get_thermal()[0], params)
        assert np.array_equal(com._engine.get_hp_levels()[0], levels)
        assert not np.array_equal(params, np.broadcast_to(np.array([21, 20, 22, 3], F32), params.shape))
        com._engine.close()


def test_hpheating_step_and_temperature_simulation_with_another_cop():
    from p2pmicrogrid_amd.dataset import ProfileDataset
    from p2pmicrogrid_amd.environment import env
    from p2pmicrogrid_amd.heating import HeatPump, HPHeating, temperature_simulation
    with _homogeneous():
        d = np.stack([np.arange(4) / 96.0, np.array([3.5, 4.0, 4.5, 5.0])], axis=1).astype(F32)
        env.setup(ProfileDataset(d, np.roll(d, -1, 0)))
        h = HPHeating(HeatPump(4.0, 3e3, 1.0), 21.0)
        h.set_state(20.25, 20.5)
        h.step()
        t_out = F32(env.temperature)
        wa, wb = temperature_step(t_out, F32(20.25), F32(20.5), F32(3e3), OracleParams(hp_cop=4.0))
        assert h.temperature[0] == wa and h.building_mass_temperature[0] == wb
        da, db = temperature_step(t_out, F32(20.25), F32(20.5), F32(3e3))
        assert (wa, wb) != (da, db)  # COP 3 gives another temperature
    rs = np.random.RandomState(1)
    t_out, t_in, t_m = (rs.uniform(lo, hi, 300).astype(F32) for lo, hi in ((-5, 25), (16, 25), (16, 25)))
    hp = rs.choice([0.0, 1500.0, 3000.0], 300).astype(F32)
    a, b = temperature_simulation(t_out, t_in, t_m, hp, hp_cop=4.0, solar_rad=50)
    wa, wb = temperature_step(t_out, t_in, t_m, hp, OracleParams(hp_cop=4.0, solar_rad=50))
    assert np.array_equal(a, wa) and np.array_equal(b, wb)
    cop = rs.choice([2.5, 3.0, 4.0], 300)
    a, b = temperature_simulation(t_out, t_in, t_m, hp, hp_cop=cop)
    wa, wb = temperature_step(t_out, t_in, t_m, hp, OracleParams(hp_cop=cop))
    assert np.array_equal(a, wa) and np.array_equal(b, wb)
