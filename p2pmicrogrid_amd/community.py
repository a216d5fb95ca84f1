"""Community orchestration (mirrors microgrid/community.py:33-423).

``CommunityMicrogrid(timeline, agents, rounds)`` keeps the reference's interface; each
``train_episode`` / ``run`` is ONE device launch (p2pmg_run_episode) over the whole episode:
negotiation rounds, market clearing, costs, rewards, TD updates and the RC update of every
agent.  Exploration is replayed from the global ``np.random`` in the reference's consumption
order, so a seeded reference script and this package draw identical
streams.  Database logging, plotting and the REST data client are out of scope.
"""
from __future__ import annotations

import collections
import os
import statistics
import time
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np

from . import database as db
from . import day_profile as dayprof
from . import dataset as ds
from . import setup
from .agent import ActingAgent, Agent, DQNAgent, GridAgent, QAgent, RuleAgent, agent_kind
from .engine import DeviceCommunityBatch, price_table, snapshot_policy_map
from .environment import env
from .heating import HeatPump, HPHeating
from .production import PV, Prosumer
from .rng import ReferenceRNG, dqn_episode_draws, python_random
from .storage import BatteryStorage, NoStorage

F32 = np.float32
ACTION_LEVELS = (0.0, 0.5, 1.0)  # agent.py:268


def thermal_arrays(agents) -> Tuple[np.ndarray, np.ndarray]:
    """What the device needs of each agent's HPHeating / HeatPump (heating.py:92-130), with the
    reference's casts: levels [N, 3] = f32(level * max_power) (heating.py:124, the product in
    Python floats) and params [N, 4] = {f32(setpoint), f32(setpoint - 1.0), f32(setpoint + 1.0),
    f32(cop)} (the bounds formed in f64 and cast afterwards, heating.py:92-94).  Pure NumPy."""
    levels = np.empty((len(agents), 3), F32)
    params = np.empty((len(agents), 4), F32)
    for i, a in enumerate(agents):
        h = a.heating
        levels[i] = [F32(l * float(h.hp.max_power)) for l in ACTION_LEVELS]
        params[i] = [F32(h._temperature_setpoint), F32(h.lower_bound), F32(h.upper_bound), F32(h.hp.cop)]
    return levels, params


def _drop_groups(profile):
    """A one-group day profile without its G axis: {"agent": {name: [P, N]}, "community": {name: [P]}}."""
    return {part: {k: v[0] for k, v in d.items()} for part, d in profile.items()}


def learning_arrays(agents) -> Tuple[np.ndarray, np.ndarray]:
    """Each agent's own QActor learning rate and discount (rl.py:58-71): (alpha [N], gamma [N]) f64,
    what DeviceCommunityBatch.set_learning takes.  Pure NumPy."""
    alpha = np.array([float(a.actor._alpha) for a in agents], np.float64)
    gamma = np.array([float(a.actor._gamma) for a in agents], np.float64)
    return alpha, gamma


def dqn_learning_arrays(agents) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Each DQNAgent's own Trainer constants (agent.py:306-311, rl.py:253-266): (gamma [N], tau [N], lr [N])
    f64, what DeviceDQNBatch.set_learning takes.  Pure NumPy."""
    gamma = np.array([float(a.trainer._gamma) for a in agents], np.float64)
    tau = np.array([float(a.trainer._tau) for a in agents], np.float64)
    lr = np.array([float(a.trainer.optimizer.learning_rate) for a in agents], np.float64)
    return gamma, tau, lr


class CommunityMicrogrid:

    def __init__(self, timeline, agents: List[ActingAgent], rounds: int, q_dtype: Optional[str] = None,
                 device: Optional[int] = None, *, battery_rule: bool = False) -> None:
        """community.py:35-43.  ``battery_rule`` (an extension, off by default): apply the battery
        rule of RuleAgent._update_storage (agent.py:138-153) to the net power of every agent that
        carries a BatteryStorage, inside the episode kernel.  The reference never calls that rule
        from an RL agent (agent.py:200-213), so by default a battery is inert, exactly as there:
        powers and costs equal the NoStorage run and the SoC stays put."""
        self.timeline = timeline
        self.time_length = len(timeline)
        self.agents = agents
        self.grid = GridAgent()
        self._rounds = rounds
        self.decisions = np.zeros((len(env), self._rounds + 1, len(self.agents)))
        self._q_dtype = q_dtype or setup.q_dtype
        self._device = setup.device if device is None else device
        self._engine: Optional[DeviceCommunityBatch] = None
        self._last_run = None  # what day_profile() reduces: the last run()'s records and the inputs it ran with
        self._uploaded: Dict[str, Any] = {}
        self._rng = ReferenceRNG()
        kinds = {agent_kind(a) for a in agents}
        if len(kinds) != 1 or None in kinds:
            raise ValueError(f"a community needs agents of one learner kind, got {kinds}")
        self._dqn = kinds == {"dqn"}
        self._rule = kinds == {"rule"}
        self._battery_rule = bool(battery_rule)
        if self._battery_rule and self._dqn:
            raise NotImplementedError("the in-kernel battery rule is supported for tabular communities")
        if self._battery_rule and self._rule:
            raise NotImplementedError("rule_episode_kernel does not apply the battery rule (the reference's "
                                      "RuleAgent.take_decision never calls _update_storage, agent.py:114-128)")

    # ------------------------------------------------------------ device state
    def _new_dqn_engine(self, T, N):
        from .dqn import DeviceDQNBatch
        old = self._engine
        carry = None
        if old is not None:  # horizon changed: carry networks, Adam state and memories over
            carry = ({w: old.get_weights(w) for w in ("adam_m", "adam_v")}, old.get_buffer(), old.step)
            for a in self.agents:
                a.actor.q_network.unbind()
                a.trainer.target_network.unbind()
            old.close()
        eng = DeviceDQNBatch(1, N, self._rounds, T, device=self._device, init_seed=None)
        for i, a in enumerate(self.agents):
            a.trainer.bind(eng, i)
        if carry is not None:
            for w, v in carry[0].items():
                eng.set_weights(w, v)
            eng.set_buffer(*carry[1])
            eng.step = carry[2]
        elif getattr(self, "_dqn_adam", None) is not None:  # train_days ran before this engine existed
            eng.set_weights("adam_m", self._dqn_adam[0])
            eng.set_weights("adam_v", self._dqn_adam[1])
            eng.step = self._dqn_adam[2]
        return eng

    def _ensure_engine(self) -> DeviceCommunityBatch:
        T, N = len(env), len(self.agents)
        if self._dqn and (self._engine is None or self._engine.T != T):
            self._engine = self._new_dqn_engine(T, N)
            self._uploaded = {}
        if self._engine is None or self._engine.T != T:
            if self._engine is not None:  # horizon changed: carry the learned tables over
                tables = self._engine.get_q()
            else:
                tables = None
            self._engine = DeviceCommunityBatch(1, N, self._rounds, T, q_dtype=self._q_dtype, device=self._device)
            for i, a in enumerate(self.agents):
                if self._rule:  # no policy to bind
                    continue
                if tables is None:
                    a.actor.bind(self._engine, i)
                else:
                    a.actor._engine = None
                    a.actor.set_qtable(tables[i])
                    a.actor.bind(self._engine, i)
            self._uploaded = {}
        eng = self._engine
        if self._uploaded.get("env") != env.version:
            time_f, t_out = env.arrays()
            eng.set_env(time_f, t_out, *price_table(time_f))
            self._uploaded["env"] = env.version
        prof_key = tuple((id(a._load), id(a.pv), id(getattr(a.pv, "pv", None) and a.pv.pv.production))
                         for a in self.agents)
        if self._uploaded.get("prof") != prof_key:
            load = np.stack([a.load_series(T) for a in self.agents])[None]
            pv = np.stack([a.pv.series(T) for a in self.agents])[None]
            eng.set_profiles(load, pv)
            eng.set_max_in(np.array([F32(a.max_in) for a in self.agents], F32)[None])
            self._uploaded["prof"] = prof_key
            self._prof_host = (np.asarray(load, F32), np.asarray(pv, F32))
        # every agent's own heat-pump levels, setpoint, comfort band and COP: keyed on the values, so
        # a change between calls (e.g. agent.heating.hp.max_power = ...) is uploaded again
        levels, params = thermal_arrays(self.agents)
        thermal_key = (levels.tobytes(), params.tobytes())
        if self._uploaded.get("thermal") != thermal_key:
            eng.set_hp_levels(levels[None])
            eng.set_thermal(params[None, :, 0], cop=params[None, :, 3], lower=params[None, :, 1],
                            upper=params[None, :, 2])
            self._uploaded["thermal"] = thermal_key
        if not (self._dqn or self._rule):
            # every actor's own alpha and gamma, keyed on the values like the thermal arrays: a change
            # between episodes (actor._alpha = ...) is uploaded again
            alpha, gamma = learning_arrays(self.agents)
            learning_key = (alpha.tobytes(), gamma.tobytes())
            if self._uploaded.get("learning") != learning_key:
                eng.set_learning(alpha=alpha[None], gamma=gamma[None])
                self._uploaded["learning"] = learning_key
        if self._dqn:
            # every trainer's own gamma, tau and learning rate, keyed on the values in the same way: a change
            # between episodes (agent.trainer._tau = ...) is uploaded again, the Adam state staying as it is
            gamma, tau, lr = dqn_learning_arrays(self.agents)
            learning_key = (gamma.tobytes(), tau.tobytes(), lr.tobytes())
            if self._uploaded.get("learning") != learning_key:
                eng.set_learning(gamma=gamma[None], tau=tau[None], lr=lr[None])
                self._uploaded["learning"] = learning_key
        return eng

    def _push_temperatures(self, eng):
        t_in = np.array([a.heating.temperature[0] for a in self.agents], F32)
        t_m = np.array([a.heating.building_mass_temperature[0] for a in self.agents], F32)
        eng.set_temperatures(t_in[None], t_m[None])
        self._push_storage(eng)

    def _batteries(self) -> List[Optional[BatteryStorage]]:
        return [a.storage if isinstance(a.storage, BatteryStorage) else None for a in self.agents]

    def _push_storage(self, eng):
        """With ``battery_rule``: capacities and SoC of the agents' batteries (NoStorage = capacity
        0) before a launch; the kernel applies the rule to every round's net power.  Without it
        nothing is uploaded (the reference's inert battery)."""
        bats = self._batteries()
        if not (self._battery_rule and any(bats)):
            if self._uploaded.get("battery"):
                eng.set_battery(None)
                self._uploaded["battery"] = False
            return
        ref = next(b for b in bats if b is not None).battery
        for b in bats:
            if b is not None and (b.battery.min_soc, b.battery.max_soc, b.battery.efficiency) != \
                    (ref.min_soc, ref.max_soc, ref.efficiency):
                raise ValueError("one community's batteries must share min_soc, max_soc and efficiency")
        cap = np.array([0.0 if b is None else b.capacity for b in bats])[None]
        soc = np.array([0.0 if b is None else b.soc for b in bats])[None]
        eng.set_battery(cap, ref.min_soc, ref.max_soc, ref.efficiency, soc0=soc)
        self._uploaded["battery"] = True

    def _pull_storage(self, eng, T: int):
        """After a launch.  The reference's inert battery: each BatteryStorage steps T times
        (storage.py:66-68), so its history holds T entries of its unchanged SoC.  With
        ``battery_rule``: the device's final SoC; the per-step SoC is not recorded on the device,
        so the history is left as it was (only the step counter advances)."""
        bats = [b for b in self._batteries() if b is not None]
        if self._uploaded.get("battery"):
            soc = eng.get_soc()[0]
            for b, x in zip(self._batteries(), soc):
                if b is not None:
                    b.set_soc(x)
                    b._time += T
            return
        for b in bats:
            for _ in range(T):
                b.step()

    def _pull_records(self, eng, T):
        act = eng.get_record("action")[:, :, 0, :]  # [T, R+1, N]
        # the power the episode simulated: the uploaded levels are these agents' (_ensure_engine)
        levels = np.array([a.heating.hp.max_power for a in self.agents])
        self.decisions = np.array(ACTION_LEVELS)[act] * levels[None, None, :]
        return act

    # ------------------------------------------------------------ the reference API
    def train_episode(self, all_rewards=None, all_losses=None, _rewards=None, _losses=None) -> Tuple[float, float]:
        """community.py:149-182: one training episode; returns (sum_t mean_i reward, mean loss)
        (the loss is 0 for tabular agents, agent.py:298)."""
        if self._dqn:
            return self._train_episode_dqn()
        if self._rule:  # community.py:160-171 calls agent.get_reward / agent.train, which RuleAgent lacks
            raise AttributeError("'RuleAgent' object has no attribute 'get_reward': rule-based communities "
                                 "only run() (agent.py:106-153)")
        eng = self._ensure_engine()
        T, N = eng.T, eng.N
        self._push_temperatures(eng)
        eps = [a.actor._epsilon for a in self.agents]
        codes = self._rng.episode_codes(T, self._rounds, N, eps)
        eng.set_replay_codes(codes)
        eng.run_episode("train", "replay", epsilon=float(eps[0]), record=("reward", "action"))
        self._pull_storage(eng, T)
        self._pull_records(eng, T)
        self.last_rewards = eng.get_record("reward")[:, 0, :]
        avg_reward = float(eng.episode_reward()[0])
        for agent in self.agents:  # reset iterators + new T0 (community.py:172-174)
            agent.reset()
        return avg_reward, 0.0

    def run(self) -> Tuple[np.ndarray, np.ndarray]:
        """community.py:95-123: greedy rollout; returns (grid + p2p power [T, N], costs [T, N])."""
        if self._rule:
            return self._run_rule()
        eng = self._ensure_engine()
        T = eng.T
        self._push_temperatures(eng)
        rec = ("grid", "p2p", "cost", "t_in", "action")
        eng.run_episode("greedy", record=rec)
        self._pull_storage(eng, T)
        r = eng.get_records(rec)
        self._keep_run(r)
        self._pull_records(eng, T)
        t_in, t_m = eng.get_temperatures()
        hist = r["t_in"][:, 0, :]
        for i, a in enumerate(self.agents):
            a.heating._history = [float(x) for x in hist[:, i]]
            a.heating._power_history = list(self.decisions[:, -1, i])
            a.heating.set_state(t_in[0, i], t_m[0, i])
        power = (r["grid"][:, 0, :] + r["p2p"][:, 0, :]).astype(F32)
        return power, r["cost"][:, 0, :]

    def summary(self, kwh: bool = False) -> Dict[str, np.ndarray]:
        """After run(): the episode's totals per agent, {name: [N] f64} for engine.SUMMARY_FIELDS (cost,
        grid and peer energy, self-consumption, discomfort, peaks), reduced on the device from the
        records run() left there (DeviceCommunityBatch.episode_summary)."""
        if self._engine is None:
            raise RuntimeError("summary() describes the last run(): call run() first")
        return {k: v[0] for k, v in self._engine.episode_summary(kwh=kwh)["agent"].items()}

    def _keep_run(self, records) -> None:
        levels, params = thermal_arrays(self.agents)
        self._last_run = (records, levels[None], *self._prof_host, params[None, :, 1], params[None, :, 2])

    def day_profile(self, period: Optional[int] = None, kwh: bool = False) -> Dict[str, Dict[str, np.ndarray]]:
        """After run(): the run by time slot, {"agent": {name: [P, N] f64}, "community": {name: [P] f64}} with
        slot(t) = t % period (None: one slot per step; e.g. 96 folds a run of several days onto one): means,
        action and discomfort shares, net flows and extrema per slot (day_profile.as_dict), from the records
        run() has already brought to the host (day_profile.from_records).  kwh: mean powers as kWh per step."""
        if self._last_run is None:
            raise RuntimeError("day_profile() describes the last run(): call run() first")
        scale = float(setup.TIME_SLOT) / 60.0 * 1e-3 if kwh else 1.0
        return _drop_groups(dayprof.as_dict(*dayprof.from_records(*self._last_run, period=period), energy_scale=scale))

    def table_stats(self) -> Dict[str, np.ndarray]:
        """Per agent: how much of its Q-table is written, its value range and its greedy-action histogram,
        {"visited", "q_min", "q_max", "abs_max": [N], "greedy": [N, n_actions]} (QActor.table_stats;
        one device pass over the community's tables once they are on the device)."""
        if self._dqn or self._rule:
            raise RuntimeError("table_stats(): only tabular (QActor) communities have Q-tables")
        if self._engine is not None and all(a.actor._engine is self._engine for a in self.agents):
            return self._engine.table_stats(0, len(self.agents))
        per = [a.actor.table_stats() for a in self.agents]
        return {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0]}

    def policy_maps(self, grid=None, q: bool = False):
        """One policy map per DQNAgent (ActorModel.policy_map): u8 [N, n0, n1, n2, n3], the greedy action
        of each agent's online network at every state of the grid; q=True: (maps, Q values f32
        [N, n0, n1, n2, n3, 3]).  One device pass over the community's networks once they are on the
        device and no grid is asked for."""
        if not self._dqn:
            raise RuntimeError("policy_maps(): only DQN communities have Q-networks (tabular: QActor.greedy_policy)")
        nets = [a.actor.q_network for a in self.agents]
        if grid is None and self._engine is not None and all(
                n._engine is self._engine and n._which == "online" and n._slot == i for i, n in enumerate(nets)):
            return self._engine.policy_map(0, len(self.agents), q=q)
        per = [a.actor.policy_map(grid=grid, q=q) for a in self.agents]
        if q:
            return np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
        return np.stack(per)

    def run_days(self, days, summary: bool = False, profile: bool = False, period: Optional[int] = None):
        """run() of this community over several days in ONE greedy launch: a per-role-table engine
        (``shared_q="role"``) with one scenario per day, holding one copy of every agent's table
        instead of one per day.  ``days``: a sequence of dicts {"time" [T], "t_out" [T], "load" [N, T],
        "pv" [N, T] (W), "t_in" [N], "t_m" [N]}, all of one length T.  Returns, per day, "power" and
        "cost" [T, N] and "decisions" [T, R + 1, N] as run() gives them, plus "t_in" [T, N] (T_in before
        each step) and "t_in_final" / "t_m_final" [N].  Each day is bit for bit what run() computes
        from that day's inputs.  The agents' tables are read, nothing else of the community changes.
        ``summary=True`` adds "summary": {name: [N] f64} per day, the day's totals per agent
        (engine.SUMMARY_FIELDS) from one device-side reduction of the launch's records.
        ``profile=True`` returns (that list, the mean day): {"agent": {name: [P, N] f64}, "community":
        {name: [P] f64}}, the days reduced per time slot and agent (day_profile.from_records on the records this
        call returns anyway, the days being the launch's scenarios; ``period``: slots, None = T).
        Tabular communities only; evaluate_days takes DQN communities too (and comes here for tabular ones)."""
        if self._rule or self._dqn:
            raise NotImplementedError("run_days needs tabular (QAgent) agents: per-role tables hold Q-tables, "
                                      "and a RuleAgent community has no policy to share")
        if self._battery_rule and any(self._batteries()):
            raise NotImplementedError("run_days does not carry battery state across days")
        D, N = len(days), len(self.agents)
        if D == 0:
            return ([], None) if profile else []
        T = len(np.asarray(days[0]["time"]).reshape(-1))

        def stack(key, shape):
            return np.stack([np.asarray(d[key], F32).reshape(shape) for d in days])
        time_f, t_out = stack("time", (T,)), stack("t_out", (T,))
        eng = DeviceCommunityBatch(D, N, self._rounds, T, q_dtype=self._q_dtype, device=self._device, shared_q="role")
        try:
            eng.set_q(np.stack([a.actor.q_table for a in self.agents]))
            eng.set_env(time_f, t_out, *price_table(time_f))
            load, pv = stack("load", (N, T)), stack("pv", (N, T))
            eng.set_profiles(load, pv)
            eng.set_max_in(np.broadcast_to(np.array([F32(a.max_in) for a in self.agents], F32), (D, N)))
            levels, params = thermal_arrays(self.agents)
            eng.set_hp_levels(np.broadcast_to(levels, (D, N, 3)))
            par = np.broadcast_to(params, (D, N, 4))
            eng.set_thermal(par[..., 0], cop=par[..., 3], lower=par[..., 1], upper=par[..., 2])
            alpha, gamma = learning_arrays(self.agents)
            eng.set_learning(alpha=np.broadcast_to(alpha, (D, N)), gamma=np.broadcast_to(gamma, (D, N)))
            eng.set_temperatures(stack("t_in", (N,)), stack("t_m", (N,)))
            rec = ("grid", "p2p", "cost", "t_in", "action")
            eng.run_episode("greedy", record=rec)
            r = eng.get_records(rec)
            t_in, t_m = eng.get_temperatures()
            totals = eng.episode_summary()["agent"] if summary else None
        finally:
            eng.close()
        return self._days_out(r, t_in, t_m, totals, levels, load, pv, par, profile, period)

    def _days_out(self, r, t_in, t_m, totals, levels, load, pv, par, profile, period):
        """What run_days / evaluate_days return, from the records [T, D, N] of the one launch, the final
        temperatures [D, N], the per-agent totals (or None) and the inputs the profile needs."""
        D, N = t_in.shape
        max_power = np.array([a.heating.hp.max_power for a in self.agents])
        out = []
        for d in range(D):
            out.append({"power": (r["grid"][:, d, :] + r["p2p"][:, d, :]).astype(F32), "cost": r["cost"][:, d, :],
                        "decisions": np.array(ACTION_LEVELS)[r["action"][:, :, d, :]] * max_power[None, None, :],
                        "t_in": r["t_in"][:, d, :], "t_in_final": t_in[d], "t_m_final": t_m[d]})
            if totals is not None:
                out[-1]["summary"] = {k: v[d] for k, v in totals.items()}
        if profile:
            arrays = dayprof.from_records(r, np.broadcast_to(levels, (D, N, 3)), load, pv, par[..., 1], par[..., 2], period=period)
            return out, _drop_groups(dayprof.as_dict(*arrays))
        return out

    def evaluate_days(self, days, summary: bool = False, profile: bool = False, period: Optional[int] = None):
        """run() of this community over several days in ONE greedy launch, for tabular and DQN communities:
        the arguments and the return value of run_days, each day bit for bit what run() computes from that
        day's inputs.  Tabular communities: run_days.  DQN communities: a DeviceDQNBatch with one scenario
        per day whose policy set is the agents' N online networks with the role map (agent i of every day
        reads network i), run by run_greedy("policy"): dqn_greedy_episode_kernel, the whole evaluation
        in one launch instead of T act launches per day.  The agents' networks are read, nothing else
        of the community changes; nothing is trained or drawn."""
        if not self._dqn:
            return self.run_days(days, summary=summary, profile=profile, period=period)
        D, N = len(days), len(self.agents)
        if D == 0:
            return ([], None) if profile else []
        T = len(np.asarray(days[0]["time"]).reshape(-1))

        def stack(key, shape):
            return np.stack([np.asarray(d[key], F32).reshape(shape) for d in days])
        time_f, t_out = stack("time", (T,)), stack("t_out", (T,))
        from .dqn import DeviceDQNBatch
        eng = DeviceDQNBatch(D, N, self._rounds, T, device=self._device, capacity=32, init_seed=None)
        try:
            eng.set_policy_nets(np.stack([a.actor.q_network.flat_weights() for a in self.agents]))
            eng.set_env(time_f, t_out, *price_table(time_f))
            load, pv = stack("load", (N, T)), stack("pv", (N, T))
            eng.set_profiles(load, pv)
            eng.set_max_in(np.broadcast_to(np.array([F32(a.max_in) for a in self.agents], F32), (D, N)))
            levels, params = thermal_arrays(self.agents)
            eng.set_hp_levels(np.broadcast_to(levels, (D, N, 3)))
            par = np.broadcast_to(params, (D, N, 4))
            eng.set_thermal(par[..., 0], cop=par[..., 3], lower=par[..., 1], upper=par[..., 2])
            eng.set_temperatures(stack("t_in", (N,)), stack("t_m", (N,)))
            rec = ("grid", "p2p", "cost", "t_in", "action")
            eng.run_greedy("policy", record=rec)
            r = eng.get_records(rec)
            t_in, t_m = eng.get_temperatures()
            totals = eng.episode_summary()["agent"] if summary else None
        finally:
            eng.close()
        return self._days_out(r, t_in, t_m, totals, levels, load, pv, par, profile, period)

    def evaluate_policies(self, days, policies, summary: bool = False, profile: bool = False,
                          period: Optional[int] = None):
        """run() of this community under K packed policy snapshots over D days, all K x D (snapshot, day) pairs
        in ONE launch of policy_episode_kernel.  ``policies``: u8 [K, N, n_states] (or [K, N, n_time, n_temp,
        n_bal, n_p2p]), K snapshots of the community's N agents in greedy_policy's order: QActor.policy_bytes()
        per checkpoint, ActorModel.policy_map() on the default grid per checkpoint, or a hand-written rule;
        bytes 0..2, or 255 for action 0.  Flat bytes are read on the grid of the agents' own tables (a DQN
        community: the default 20^4 map grid) and refused with the reason when they do not fit it; 6-D input
        carries its grid.  ``days`` as for evaluate_days.  Scenario k * D + d is day d under
        snapshot k, and its agent i reads policy k * N + i (engine.snapshot_policy_map).
        Returns a list of K lists of D dicts, each what evaluate_days returns for that day when the agents hold
        snapshot k's tables, bit for bit; ``summary=True`` adds the device summaries.  ``profile=True`` returns
        (that, the day profile with groups = snapshot index): {"agent": {name: [K, P, N] f64}, "community":
        {name: [K, P] f64}}, so a validation curve with its day-to-day spread comes back as K rows.
        The engine is a ``shared_q=True`` context: ONE table, which the launch never reads, so memory is
        K * N * n_states bytes of policies plus inputs and records, and does not grow with A * 5 MB of tables.
        Nothing of the community changes.  The agents' thermal values, heat-pump levels and max_in are used;
        the policies need not come from them."""
        if self._rule:
            raise TypeError("evaluate_policies: a RuleAgent community has no policy to replace")
        if self._battery_rule and any(self._batteries()):
            raise NotImplementedError("evaluate_policies does not carry battery state across days")
        D, N = len(days), len(self.agents)
        pol = np.asarray(policies)
        if pol.dtype != np.uint8 or pol.ndim < 3 or pol.shape[1] != N:
            raise ValueError(f"policies must be uint8 [K, {N}, n_states], got {pol.dtype} {pol.shape}")
        K = int(pol.shape[0])
        if D == 0 or K == 0:
            return ([], None) if profile else []
        T = len(np.asarray(days[0]["time"]).reshape(-1))
        S = K * D
        # the table grid the bytes were made on: the policies' own axes, else the agents' tables' (a tabular
        # community; its actors share one shape), else the default 20^4 (a DQN community's default map grid)
        if pol.ndim == 6:
            grid = tuple(int(x) for x in pol.shape[2:])
        elif pol.ndim != 3:
            raise ValueError(f"policies must be [K, {N}, n_states] or [K, {N}, n_time, n_temp, n_bal, n_p2p], got {pol.shape}")
        else:
            shapes = {tuple(int(x) for x in a.actor._shape[:4]) for a in self.agents if hasattr(a.actor, "_shape")}
            if len(shapes) > 1:
                raise ValueError(f"evaluate_policies: the agents' tables differ in shape ({sorted(shapes)}); give the "
                                 "policies with their grid axes")
            grid = shapes.pop() if shapes else (20, 20, 20, 20)
            if int(np.prod(grid)) != pol.shape[2]:
                raise ValueError(f"evaluate_policies: flat policies of {pol.shape[2]} states do not fit the grid "
                                 f"{grid} ({int(np.prod(grid))} states): give them as [K, {N}, n_time, n_temp, n_bal, n_p2p]")
        dims = dict(zip(("n_time_states", "n_temp_states", "n_balance_states", "n_p2p_states"), grid))
        pol = np.ascontiguousarray(pol.reshape(K * N, -1))

        def stack(key, shape):  # [D, ...] -> [K * D, ...], day d of every snapshot
            return np.tile(np.stack([np.asarray(d[key], F32).reshape(shape) for d in days]), (K,) + (1,) * len(shape))
        time_f, t_out = stack("time", (T,)), stack("t_out", (T,))
        eng = DeviceCommunityBatch(S, N, self._rounds, T, q_dtype="f32", device=self._device, shared_q=True, **dims)
        try:
            eng.set_policy_set(pol, policy_of=snapshot_policy_map(K, D, N))
            eng.set_env(time_f, t_out, *price_table(time_f))
            load, pv = stack("load", (N, T)), stack("pv", (N, T))
            eng.set_profiles(load, pv)
            eng.set_max_in(np.broadcast_to(np.array([F32(a.max_in) for a in self.agents], F32), (S, N)))
            levels, params = thermal_arrays(self.agents)
            eng.set_hp_levels(np.broadcast_to(levels, (S, N, 3)))
            par = np.broadcast_to(params, (S, N, 4))
            eng.set_thermal(par[..., 0], cop=par[..., 3], lower=par[..., 1], upper=par[..., 2])
            eng.set_temperatures(stack("t_in", (N,)), stack("t_m", (N,)))
            rec = ("grid", "p2p", "cost", "t_in", "action")
            eng.run_policy(record=rec)
            r = eng.get_records(rec)
            t_in, t_m = eng.get_temperatures()
            totals = eng.episode_summary()["agent"] if summary else None
            prof = eng.day_profile(period=period, groups=np.repeat(np.arange(K), D), n_groups=K, as_dict=True) if profile else None
        finally:
            eng.close()
        flat = self._days_out(r, t_in, t_m, totals, levels, load, pv, par, False, period)
        out = [flat[k * D:(k + 1) * D] for k in range(K)]
        return (out, prof) if profile else out

    def _role_engine(self, days):
        """The role engine of train_days: D scenarios (the days) x N agents, shared="role", built the way
        evaluate_days builds its batch.  Kept between calls while the days and the agents' thermal values stay
        the same (its replay rings are then already filled); -> (engine, t_in [D, N], t_m [D, N], new)."""
        from .dqn import DeviceDQNBatch
        D, N = len(days), len(self.agents)
        T = len(np.asarray(days[0]["time"]).reshape(-1))

        def stack(key, shape):
            return np.stack([np.asarray(d[key], F32).reshape(shape) for d in days])
        time_f, t_out = stack("time", (T,)), stack("t_out", (T,))
        load, pv = stack("load", (N, T)), stack("pv", (N, T))
        t_in, t_m = stack("t_in", (N,)), stack("t_m", (N,))
        max_in = np.array([F32(a.max_in) for a in self.agents], F32)
        levels, params = thermal_arrays(self.agents)
        capacity = int(self.agents[0].trainer.buffer.buffer_size)
        key = (D, N, T, self._rounds, capacity) + tuple(x.tobytes() for x in (time_f, t_out, load, pv, t_in, t_m, max_in,
                                                                           levels, params))
        kept = getattr(self, "_role", None)
        if kept is not None and kept[0] == key:
            return kept[1], t_in, t_m, False
        if kept is not None:
            kept[1].close()
            self._role = None
        eng = DeviceDQNBatch(D, N, self._rounds, T, shared="role", device=self._device, capacity=capacity, init_seed=None)
        try:
            eng.set_env(time_f, t_out, *price_table(time_f))
            eng.set_profiles(load, pv)
            eng.set_max_in(np.broadcast_to(max_in, (D, N)))
            eng.set_hp_levels(np.broadcast_to(levels, (D, N, 3)))
            par = np.broadcast_to(params, (D, N, 4))
            eng.set_thermal(par[..., 0], cop=par[..., 3], lower=par[..., 1], upper=par[..., 2])
        except BaseException:
            eng.close()
            raise
        self._role = (key, eng)
        self._role_episode = 0
        return eng, t_in, t_m, True

    def train_days(self, days, episodes: int = 1, fill: Optional[int] = None) -> List[Tuple[float, float]]:
        """Train this DQN community over several days at once: the D days are the D scenarios of ONE role
        engine (DeviceDQNBatch(shared="role")), whose N networks are the agents' and learn from agent i of every
        day in each env step (include/p2pmg.h, p2pmg_dqn_setup_roles), instead of D train_episode calls of one
        scenario each.  ``days`` as for evaluate_days.  The agents' online and target networks, Adam moments and
        iteration count are uploaded as the N role networks; on the first call for these days ``fill`` Philox
        fill episodes (None: 5, init_buffers' count) load the engine's own replay rings, one per day and
        agent; then ``episodes`` Philox training episodes run at the actors' current epsilon (one rate for
        the launch: the actors' rates must be equal), every episode from the days' starting temperatures.
        Epsilon is not decayed here: the reference's cadence (community.py main) stays with the caller.
        Networks, Adam state and counts are written back into the agents, so evaluate_days, run, policy_maps
        and save_to_file see the trained networks.  Returns, per training episode, (the mean over the days of
        sum_t mean_i r, the mean loss).  Draws come from the engine's Philox streams, not np.random."""
        if self._rule:
            raise TypeError("train_days: a RuleAgent community has nothing to train")
        if not self._dqn:
            raise TypeError("train_days trains DQN communities; a tabular community trains over many days on "
                            "DeviceCommunityBatch(shared_q=\"role\") (see run_days)")
        if len(days) == 0 or episodes < 0:
            raise ValueError("train_days needs at least one day and episodes >= 0")
        eps = [float(a.actor._epsilon) for a in self.agents]
        if len(set(eps)) != 1:
            raise ValueError(f"train_days explores at one rate per launch; the actors' rates differ: {eps}")
        N = len(self.agents)
        # the Adam state: the community engine's (the trainers are bound to it) or what the last call left
        ceng = self._engine
        if ceng is not None:
            steps = ceng.net_steps()
            if len(set(int(s) for s in steps)) != 1:
                raise NotImplementedError("train_days needs one Adam iteration count for every agent")
            adam = (ceng.get_weights("adam_m"), ceng.get_weights("adam_v"), int(steps[0]))
        else:
            adam = getattr(self, "_dqn_adam", None) or (np.zeros((N, 4609), F32), np.zeros((N, 4609), F32), 0)
        eng, t_in, t_m, new = self._role_engine(days)
        eng.set_weights("online", np.stack([a.actor.q_network.flat_weights() for a in self.agents]))
        eng.set_weights("target", np.stack([a.trainer.target_network.flat_weights() for a in self.agents]))
        eng.set_weights("adam_m", adam[0])
        eng.set_weights("adam_v", adam[1])
        eng.step = adam[2]
        gamma, tau, lr = dqn_learning_arrays(self.agents)
        eng.set_learning(gamma=gamma, tau=tau, lr=lr)
        for _ in range((5 if fill is None else int(fill)) if new else 0):
            eng.set_temperatures(t_in, t_m)
            eng.run_episode("fill", "philox", episode=self._role_episode, epsilon=eps[0])
            self._role_episode += 1
        out = []
        for _ in range(int(episodes)):
            eng.set_temperatures(t_in, t_m)
            eng.run_episode("train", "philox", episode=self._role_episode, epsilon=eps[0], record=("loss",))
            self._role_episode += 1
            out.append((float(np.mean(eng.episode_reward(), dtype=np.float32)),
                        float(np.mean(eng.get_record("loss"), dtype=np.float32))))
        online, target = eng.get_weights("online"), eng.get_weights("target")
        self._dqn_adam = (eng.get_weights("adam_m"), eng.get_weights("adam_v"), int(eng.net_steps()[0]))
        for i, a in enumerate(self.agents):
            a.actor.q_network.set_flat_weights(online[i])
            a.trainer.target_network.set_flat_weights(target[i])
        if ceng is not None:
            ceng.set_weights("adam_m", self._dqn_adam[0])
            ceng.set_weights("adam_v", self._dqn_adam[1])
            ceng.step = self._dqn_adam[2]
        return out

    def _run_rule(self) -> Tuple[np.ndarray, np.ndarray]:
        """run() of a RuleAgent community: one rule_episode_kernel launch (R = 0)."""
        if self._rounds != 0:
            raise ValueError("RuleAgent communities run with rounds = 0: with more rounds the reference's "
                             "tensor_diag_part on the (N, 1) proposal stack fails (community.py:76)")
        eng = self._ensure_engine()
        self._push_temperatures(eng)
        eng.set_hp_state(np.array([float(np.asarray(a.heating.hp.power).reshape(-1)[0]) for a in self.agents], F32)[None])
        rec = ("grid", "p2p", "cost", "t_in", "action")
        eng.run_rule_episode(record=rec)
        r = eng.get_records(rec)
        self._keep_run(r)
        self._pull_records(eng, eng.T)
        t_in, t_m = eng.get_temperatures()
        on = eng.get_hp_state()[0]
        hist = r["t_in"][:, 0, :] if r["t_in"].ndim == 3 else r["t_in"]
        for i, a in enumerate(self.agents):
            a.heating._history = [float(x) for x in hist[:, i]]
            a.heating._power_history = list(self.decisions[:, -1, i])
            a.heating.set_state(t_in[0, i], t_m[0, i])
            a.heating.hp.power = float(on[i])
        power = (r["grid"][:, 0, :] + r["p2p"][:, 0, :]).astype(F32)
        return power, r["cost"][:, 0, :]

    # ------------------------------------------------------------ DQN agents
    def _counts(self, eng):
        _, added = eng.get_buffer()
        return np.minimum(added, eng.capacity)

    def _train_episode_dqn(self) -> Tuple[float, float]:
        eng = self._ensure_engine()
        T, N = eng.T, eng.N
        self._push_temperatures(eng)
        eps = [a.actor._epsilon for a in self.agents]
        codes, samples = dqn_episode_draws(python_random(), self._rng.rs, T, self._rounds, N, eps,
                                           counts=self._counts(eng))
        eng.set_replay_codes(codes)
        eng.set_samples(samples)
        eng.run_episode("train", "replay", epsilon=float(eps[0]), record=("reward", "action", "loss"))
        self._pull_records(eng, T)
        self.last_rewards = eng.get_record("reward")[:, 0, :]
        self.last_losses = eng.get_record("loss")[:, 0, :]
        avg_reward = float(eng.episode_reward()[0])
        for agent in self.agents:
            agent.reset()
        return avg_reward, float(np.mean(self.last_losses, dtype=np.float32))

    def init_buffers(self) -> None:
        """community.py:125-147: five episodes of memory with the exploring actors (no training),
        then Trainer.initialize_target per agent.  Tabular agents have no memory."""
        if not self._dqn:
            return
        eng = self._ensure_engine()
        T, N = eng.T, eng.N
        for _ in range(5):
            self._push_temperatures(eng)
            eps = [a.actor._epsilon for a in self.agents]
            codes, _ = dqn_episode_draws(python_random(), self._rng.rs, T, self._rounds, N, eps)
            eng.set_replay_codes(codes)
            eng.run_episode("fill", "replay", epsilon=float(eps[0]))
            for agent in self.agents:
                agent.reset()
        for agent in self.agents:
            agent.trainer.initialize_target()

    # ------------------------------------------------------------ per-step API (host glue)
    # For callers that step the community themselves, as community.py:149-182 does: the same
    # TF op order on f32 host values (canonical sequential sums), with the agents'
    # per-step methods calling the device for the learner and the RC update.
    def _assign_powers(self, p2p_power) -> Tuple[np.ndarray, np.ndarray]:
        """community.py:45-54: opposite-sign pairs exchange min(|P_ij|, |P_ji|), the rest is grid."""
        P = np.asarray(p2p_power, F32)
        p_match = np.where(np.sign(P) != np.sign(P.T), P, F32(0.0)).astype(F32)
        exchange = (np.sign(p_match) * np.minimum(np.abs(p_match), np.abs(p_match).T)).astype(F32)
        diff = (P - exchange).astype(F32)
        p_grid = np.zeros(P.shape[0], F32)
        p_p2p = np.zeros(P.shape[0], F32)
        for j in range(P.shape[1]):
            p_grid = (p_grid + diff[:, j]).astype(F32)
            p_p2p = (p_p2p + exchange[:, j]).astype(F32)
        return p_grid, p_p2p

    def _compute_costs(self, grid_power, peer_power, buying_price, injection_price, p2p_price) -> np.ndarray:
        """community.py:56-65 (prices [T] or scalars; powers [..., N])."""
        g, pp = np.asarray(grid_power, F32), np.asarray(peer_power, F32)
        buy = np.asarray(buying_price, F32).reshape(-1)[:, None]
        inj = np.asarray(injection_price, F32).reshape(-1)[:, None]
        p2p = np.asarray(p2p_price, F32).reshape(-1)[:, None]
        c = (np.where(g >= F32(0.0), g * buy, g * inj) + pp * p2p).astype(F32)
        return ((((c * F32(setup.TIME_SLOT)) / F32(setup.MINUTES_PER_HOUR)).astype(F32)) * F32(1e-3)).astype(F32)

    def _run(self, time: int, state, training: bool = False):
        """community.py:67-93: prices, R + 1 Jacobi negotiation rounds (each agent answers the
        previous round's column, diagonal zeroed), market clearing on the final proposals."""
        st = np.asarray(state.numpy() if hasattr(state, "numpy") else state, F32).reshape(-1)
        buying_price, injection_price = self.grid.take_decision(st)
        p2p_price = ((F32(buying_price) + np.asarray(injection_price, F32)) / F32(2)).astype(F32)
        N = len(self.agents)
        P = np.zeros((N, N), F32)
        for r in range(self._rounds + 1):
            P = (P - np.diag(np.diag(P))).astype(F32)
            rows = []
            for i, agent in enumerate(self.agents):
                col = (-P[:, i]).astype(F32)
                if training:
                    action, _ = agent(st[None], col)
                else:
                    action, _ = agent.take_decision(st[None], col)
                rows.append(np.asarray(action, F32).reshape(-1))
            P = np.stack(rows).astype(F32)
            for a, agent in enumerate(self.agents):
                self.decisions[time, r, a] = float(agent.heating.power[0])
        p_grid, p_p2p = self._assign_powers(P)
        return p_grid, p_p2p, F32(buying_price), np.asarray(injection_price, F32), p2p_price

    def _step(self) -> None:
        for agent in self.agents:
            agent.step()
        self.grid.step()

    def reset(self) -> None:
        for agent in self.agents:
            agent.reset()
        self.grid.reset()
        self.decisions = np.zeros((len(env), self._rounds + 1, len(self.agents)))


def get_community(agent_constructor: Callable[..., ActingAgent], n_agents: int,
                  homogeneous: bool = False, rounds_: Optional[int] = None) -> CommunityMicrogrid:
    """community.py:198-234 with the same np.random consumption (ratings, then per agent
    HPHeating T_m, T_in) and the same derived quantities."""
    env_df, agent_dfs = ds.get_train_data()
    if homogeneous:
        agent_dfs = [agent_dfs[0]] * n_agents
    timeline = env_df['time'].map(lambda t: int(t * setup.MINUTES_PER_HOUR / setup.TIME_SLOT * setup.HOURS_PER_DAY))
    agents: List[ActingAgent] = []
    rng = ReferenceRNG()
    load_ratings, pv_ratings = rng.community_ratings(n_agents, homogeneous)
    Agent.reset_ids()
    for i in range(n_agents):
        max_power = max(load_ratings[i], pv_ratings[i])
        safety = 1.1
        agent_load = ds.dataframe_to_dataset(agent_dfs[i % len(agent_dfs)]['load'] * load_ratings[i] * 1e3)
        agent_pv = ds.dataframe_to_dataset(agent_dfs[i % len(agent_dfs)]['pv'] * pv_ratings[i] * 1e3)
        agents.append(agent_constructor(agent_load,
                                        Prosumer(PV(peak_power=pv_ratings[i] * 1e3, production=agent_pv)),
                                        NoStorage(),
                                        HPHeating(HeatPump(cop=3.0, max_power=3 * 1e3, power=0.0), 21.0, rng=rng),
                                        max_in=max_power * safety * 1e3,
                                        max_out=-(max_power + safety * 1e3)))
    env.setup(ds.dataframe_to_dataset(env_df))
    return CommunityMicrogrid(timeline, agents, setup.rounds if rounds_ is None else rounds_)


def get_rule_based_community(n_agents: int, homogeneous: bool) -> CommunityMicrogrid:
    """community.py:237-238, with rounds = 0: a RuleAgent ignores the proposals, and with more
    rounds the reference's run() fails on the (N, 1) proposal stack (tensor_diag_part)."""
    return get_community(RuleAgent, n_agents, homogeneous=homogeneous, rounds_=0)


def get_rl_based_community(n_agents: int, homogeneous: bool) -> CommunityMicrogrid:
    """community.py:240-245"""
    if setup.implementation == 'tabular':
        return get_community(QAgent, n_agents, homogeneous=homogeneous)
    if setup.implementation == 'dqn':
        return get_community(DQNAgent, n_agents, homogeneous=homogeneous)
    raise ValueError(f"unknown implementation {setup.implementation!r}")


def setting_name(nr_agents=None, rounds=None, homogeneous=None) -> str:
    """community.py:423"""
    n = setup.nr_agents if nr_agents is None else nr_agents
    r = setup.rounds if rounds is None else rounds
    h = setup.homogeneous if homogeneous is None else homogeneous
    return f'{n}-multi-agent-com-rounds-{r}-{"homo" if h else "hetero"}'


def _set_day_profiles(community: CommunityMicrogrid, agent_dfs, rows=None) -> None:
    """community.py:306-311 / :386-391: each agent's load and PV of the evaluation data, scaled by
    the homogeneous ratings or by fresh N(0.7, 0.2) / N(4, 0.2) draws (load first, then PV, per
    agent: the reference's np.random consumption order)."""
    for i, agent in enumerate(community.agents):
        df = agent_dfs[i] if rows is None else agent_dfs[i].loc[rows]
        agent_load = ds.dataframe_to_dataset(df['load'] * (0.7e3 if setup.homogeneous
                                                           else np.random.normal(0.7, 0.2, 1) * 1e3))
        agent_pv = ds.dataframe_to_dataset(df['pv'] * (4e3 if setup.homogeneous
                                                       else np.random.normal(4, 0.2, 1) * 1e3))
        agent.set_profiles(agent_load, agent_pv)


def main(con=None, load_agents: bool = False, analyse: bool = False, *, episodes: Optional[int] = None,
         save: bool = True, verbose: bool = True) -> Dict[str, Any]:
    """community.py:248-321 (same positional signature: ``main(db_connection, load_agents=True,
    analyse=True)`` as at community.py:436).  Episodes ``setup.starting_episodes`` ..
    ``setup.max_episodes`` (``episodes`` = a shorter run), epsilon decay after episodes 0, 50, ...,
    running means to ``training_progress`` (db.log_training_progress) when a connection is given,
    ``.npy`` checkpoints every ``setup.save_episodes`` and at the end.  ``analyse`` runs the
    reference's greedy validation rollout (community.py:302-316: validation split, fresh rating
    draws, community.run) and returns its power/cost; the plots of analyse_community_output
    (data_analysis.py, out of scope) and save_times' ../data JSON are not produced."""
    setting = setting_name()
    if verbose:
        print(setting)
    community = get_rl_based_community(setup.nr_agents, homogeneous=setup.homogeneous)
    if load_agents:
        for agent in community.agents:
            agent.load_from_file(setting, setup.implementation)
    if setup.implementation == 'dqn':
        community.init_buffers()  # community.py:265-267
    rewards_q: collections.deque = collections.deque(maxlen=setup.min_episodes_criterion)
    errors_q: collections.deque = collections.deque(maxlen=setup.min_episodes_criterion)
    history = []
    t0 = time.time()
    last = setup.max_episodes if episodes is None else setup.starting_episodes + episodes
    for episode in range(setup.starting_episodes, last):
        reward, error = community.train_episode()
        rewards_q.append(reward)
        errors_q.append(error)
        history.append(reward)
        if episode % setup.min_episodes_criterion == 0:
            if verbose:
                print(f'Average reward: {statistics.mean(rewards_q):.3f}. '
                      f'Average error: {statistics.mean(errors_q):.3f}')
            for agent in community.agents:
                agent.actor.decay_exploration()
            db.log_training_progress(con, setting, setup.implementation, episode, statistics.mean(rewards_q),
                                     statistics.mean(errors_q))
        if save and (episode + 1) % setup.save_episodes == 0:
            for agent in community.agents:
                agent.save_to_file(setting, setup.implementation)
    if history:
        db.log_training_progress(con, setting, setup.implementation, last - 1, statistics.mean(rewards_q),
                                 statistics.mean(errors_q))
    if save:
        for agent in community.agents:
            agent.save_to_file(setting, setup.implementation)
    out: Dict[str, Any] = {"community": community, "rewards": history, "train_time": time.time() - t0}
    if analyse:  # community.py:302-316
        env_df, agent_dfs = ds.get_validation_data()
        env.setup(ds.dataframe_to_dataset(env_df))
        _set_day_profiles(community, agent_dfs)
        t_run = time.time()
        power, cost = community.run()
        out.update(run_time=time.time() - t_run, power=power, cost=cost,
                   cost_per_agent=np.sum(cost, axis=0, dtype=np.float32), decisions=community.decisions.copy())
    return out


def save_community_results(con, is_testing: bool, setting: str, day: int, community: CommunityMicrogrid,
                           cost: np.ndarray) -> None:
    """community.py:333-353: one test/validation row per agent-step (time, load, pv, T_in, heat-pump
    power, cost) and, for test runs, the heat-pump decision of every negotiation round."""
    time_f, _ = env.arrays()
    T = len(time_f)
    times = [float(x) for x in time_f]
    days = [int(day)] * T
    impl = setup.implementation
    for i, agent in enumerate(community.agents):
        row = (agent.load_series(T), agent.pv.series(T), agent.heating.get_history(),
               agent.heating._power_history, cost[:, i])
        if is_testing:
            db.log_test_results(con, setting, i, days, times, *row, impl)
        else:
            db.log_validation_results(con, setting, i, days, times, *row, impl)
    if is_testing:
        for a in range(len(community.agents)):
            for r in range(community._rounds + 1):
                db.log_rounds_decision(con, setting, a, days, times, r, community.decisions[:, r, a].tolist())


def load_and_run(con=None, is_testing: bool = False, analyse: bool = True) -> Dict[int, Dict[str, np.ndarray]]:
    """community.py:364-412 (same signature: ``load_and_run(db_connection, is_testing=True,
    analyse=False)`` as at community.py:437): greedy evaluation per test/validation day from the
    saved tables, a fresh start each day; rows go to the DB when a connection is given
    (save_community_results); returns per-day power, cost and decisions.  ``analyse`` would only
    plot (data_analysis.py, out of scope), so it changes nothing here."""
    setting = setting_name()
    community = get_rl_based_community(setup.nr_agents, homogeneous=setup.homogeneous)
    for agent in community.agents:
        agent.load_from_file(setting, setup.implementation)
    env_df, agent_dfs = ds.get_test_data() if is_testing else ds.get_validation_data()
    days = np.unique(env_df['day'])
    day_indices = {day: env_df['day'] == day for day in days}
    env_df = env_df.drop(axis=1, labels='day')
    if setup.homogeneous:
        agent_dfs = [agent_dfs[0]] * setup.nr_agents
    out = {}
    for day in days:
        env.setup(ds.dataframe_to_dataset(env_df[day_indices[day]]))
        community.reset()
        _set_day_profiles(community, agent_dfs, day_indices[day])
        power, cost = community.run()
        if con is not None:
            save_community_results(con, is_testing, setting, int(day), community, np.asarray(cost))
        out[int(day)] = {"power": power, "cost": cost, "decisions": community.decisions.copy()}
    return out


def load_and_run_batched(con=None, is_testing: bool = False) -> Dict[int, Dict[str, np.ndarray]]:
    """load_and_run with every day in ONE greedy launch (CommunityMicrogrid.evaluate_days): the same per-day
    results, bit for bit, the same DB rows and the same np.random consumption.  The day-by-day loop
    draws, per day, community.reset()'s T0 and then _set_day_profiles' scales and resets; the greedy
    launch draws nothing, so all of that is drawn first, day after day in that order, and each day's
    inputs are kept for the launch.  Tabular (per-role tables) and DQN (a policy set of the agents'
    networks) communities."""
    setting = setting_name()
    community = get_rl_based_community(setup.nr_agents, homogeneous=setup.homogeneous)
    for agent in community.agents:
        agent.load_from_file(setting, setup.implementation)
    env_df, agent_dfs = ds.get_test_data() if is_testing else ds.get_validation_data()
    days = np.unique(env_df['day'])
    day_indices = {day: env_df['day'] == day for day in days}
    env_df = env_df.drop(axis=1, labels='day')
    if setup.homogeneous:
        agent_dfs = [agent_dfs[0]] * setup.nr_agents
    inputs, held = [], []
    for day in days:
        day_env = ds.dataframe_to_dataset(env_df[day_indices[day]])
        env.setup(day_env)
        community.reset()
        _set_day_profiles(community, agent_dfs, day_indices[day])
        time_f, t_out = env.arrays()
        T = len(time_f)
        inputs.append({"time": time_f, "t_out": t_out,
                       "load": np.stack([a.load_series(T) for a in community.agents]),
                       "pv": np.stack([a.pv.series(T) for a in community.agents]),
                       "t_in": np.array([a.heating.temperature[0] for a in community.agents], F32),
                       "t_m": np.array([a.heating.building_mass_temperature[0] for a in community.agents], F32)})
        held.append((day_env, [(a._load, a.pv.pv.production) for a in community.agents]))
    results = community.evaluate_days(inputs)
    out = {}
    for day, (day_env, profiles), res in zip(days, held, results):
        # the community as run() leaves it after this day: what save_community_results reads
        env.setup(day_env)
        community.decisions = res["decisions"]
        for i, (a, (load, pv)) in enumerate(zip(community.agents, profiles)):
            a._load, a.pv.pv.production = load, pv
            a.heating._history = [float(x) for x in res["t_in"][:, i]]
            a.heating._power_history = list(res["decisions"][:, -1, i])
            a.heating.set_state(res["t_in_final"][i], res["t_m_final"][i])
        if con is not None:
            save_community_results(con, is_testing, setting, int(day), community, np.asarray(res["cost"]))
        out[int(day)] = {"power": res["power"], "cost": res["cost"], "decisions": res["decisions"].copy()}
    return out
