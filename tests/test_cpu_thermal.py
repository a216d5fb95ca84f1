"""Per-agent heat-pump size, COP and comfort setpoint: the host-side pieces (no GPU)."""
from types import SimpleNamespace

import numpy as np

from p2pmicrogrid_amd import _lib
from p2pmicrogrid_amd.community import thermal_arrays
from p2pmicrogrid_amd.heating import HeatPump

F32 = np.float32


def _agent(cop, max_power, setpoint):
    """What thermal_arrays reads of an agent: its HPHeating's pump, setpoint and bounds (the bounds
    as HPHeating.__init__ forms them, heating.py:92-94: Python floats)."""
    heating = SimpleNamespace(hp=HeatPump(cop, max_power, 0.0), _temperature_setpoint=setpoint,
                              lower_bound=setpoint - 1.0, upper_bound=setpoint + 1.0)
    return SimpleNamespace(heating=heating)


def test_thermal_arrays_use_the_reference_casts():
    agents = [_agent(2.5, 2e3, 19.5), _agent(3.0, 3e3, 21.3), _agent(4.0, 5e3, 22.0)]
    levels, params = thermal_arrays(agents)
    assert levels.dtype == F32 and params.dtype == F32
    assert levels.shape == (3, 3) and params.shape == (3, 4)
    assert np.array_equal(levels, np.array([[0.0, 1e3, 2e3], [0.0, 1.5e3, 3e3], [0.0, 2.5e3, 5e3]], F32))
    want = np.array([[F32(19.5), F32(19.5 - 1.0), F32(19.5 + 1.0), F32(2.5)],
                     [F32(21.3), F32(21.3 - 1.0), F32(21.3 + 1.0), F32(3.0)],
                     [F32(22.0), F32(22.0 - 1.0), F32(22.0 + 1.0), F32(4.0)]], F32)
    assert np.array_equal(params, want)
    # the bound is formed in f64 and cast afterwards (heating.py:92-94)
    assert params[1, 1] == F32(21.3 - 1.0)


def test_bounds_are_cast_after_the_f64_subtraction():
    """Where the order of cast and subtraction matters: 16.3 - 1 leaves f32(16.3)'s binade, so the
    f32 subtraction keeps the coarser grid's rounding error and the f64 one does not.  (Between 17
    and 31 the two agree: both results lie in [16, 32).)"""
    assert F32(16.3 - 1.0) != F32(16.3) - F32(1)
    _, params = thermal_arrays([_agent(3.0, 3e3, 16.3)])
    assert params[0, 1] == F32(16.3 - 1.0)
    assert params[0, 2] == F32(16.3 + 1.0)


def test_thermal_arrays_of_hpheating_objects():
    """The same through the real HPHeating (homogeneous: no T0 draws from np.random)."""
    from p2pmicrogrid_amd import setup
    from p2pmicrogrid_amd.heating import HPHeating
    was = setup.homogeneous
    setup.homogeneous = True
    try:
        agents = [SimpleNamespace(heating=HPHeating(HeatPump(4.0, 5e3, 0.0), 21.3))]
    finally:
        setup.homogeneous = was
    levels, params = thermal_arrays(agents)
    assert np.array_equal(levels, np.array([[0.0, 2.5e3, 5e3]], F32))
    assert np.array_equal(params, np.array([[F32(21.3), F32(21.3 - 1.0), F32(21.3 + 1.0), F32(4.0)]], F32))


def test_abi_version_and_new_symbols():
    assert _lib.ABI_VERSION == 9
    L = _lib.lib()
    assert L.p2pmg_abi_version() == 9
    for name in ("p2pmg_set_thermal", "p2pmg_get_thermal", "p2pmg_rc_step_ex"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None, name
