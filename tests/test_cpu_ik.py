"""BatchedSim.solve_ik without a device: the C ABI's symbols, layout and first refusals, the method's ValueErrors, the condition tests/ik_cases.py puts on its targets."""
import ctypes

import numpy as np
import pytest

import gymnasium_robotics_amd as grx
import ik_cases as I
from gymnasium_robotics_amd import _native


def test_layout_mirrors_the_struct():
    want = [ctypes.sizeof(_native.SimIkStruct)] + [getattr(_native.SimIkStruct, f).offset for f, _ in _native.SimIkStruct._fields_]
    got = (ctypes.c_longlong * len(want))()
    assert _native.lib().grx_sim_ik_layout(got, len(want)) == len(want) == 19 and list(got) == want and {"grx_sim_ik", "grx_sim_ik_layout"} <= set(_native.EXPORTED_SYMBOLS)


@pytest.mark.parametrize("kw, n_worlds, message", [
    (None, 1, "null argument block"), (dict(qpos0=None), 1, "null qpos0 / target_pos / site"), (dict(target_pos=None), 1, "null qpos0 / target_pos / site"),
    (dict(site=None), 1, "null qpos0 / target_pos / site"), (dict(qpos=None), 1, "null outputs (qpos, err, iters)"), (dict(err=None), 1, "null outputs (qpos, err, iters)"),
    (dict(iters=None), 1, "null outputs (qpos, err, iters)"), ({}, 0, "n_worlds < 1"), (dict(n_sites=0), 1, "n_sites = 0 is outside 1 .. 4"),
    (dict(n_sites=5), 1, "n_sites = 5 is outside 1 .. 4"), (dict(max_iters=-1), 1, "max_iters < 0"), (dict(damping=0.0), 1, "damping <= 0"),
    (dict(damping=float("nan")), 1, "damping <= 0"), (dict(tol=-1e-9), 1, "tol < 0"), (dict(max_step=0.0), 1, "max_step <= 0")])
def test_refusals_that_precede_the_model(kw, n_worlds, message):
    """these checks read nothing of the model, so a dummy non-NULL handle reaches them; the ones that read it (site range, origin, shift group) are in tests/test_gpu_ik.py"""
    L, dummy, words, site = _native.lib(), ctypes.create_string_buffer(1 << 16), (ctypes.c_float * 64)(), (ctypes.c_int * 4)()
    p = ctypes.addressof(words)
    full = dict(qpos0=p, target_pos=p, qpos=p, err=p, iters=p, site=ctypes.addressof(site), n_sites=1, max_iters=4, damping=0.01, max_step=0.5, tol=1e-4, rot_weight=1.0)
    assert L.grx_sim_ik(None, ctypes.byref(_native.SimIkStruct(**full)), 1, None) == -1 and L.grx_last_error().decode() == "grx_sim_ik: null model"
    assert L.grx_sim_ik(ctypes.addressof(dummy), None if kw is None else ctypes.byref(_native.SimIkStruct(**dict(full, **kw))), n_worlds, None) == -1
    assert L.grx_last_error().decode() == "grx_sim_ik: " + message


def test_value_errors_without_a_device():
    sim = grx.BatchedSim(I.model("tree"), num_worlds=3)
    tp = np.zeros((3, 1, 3), np.float32)
    for args, kw in ((("left", tp.astype(np.float64)), {}), (("left", tp[:2]), {}), ((("left", "right"), tp), {}), (("left", tp), dict(target_quat=np.zeros((3, 1, 3), np.float32))),
                     (("left", tp), dict(qpos0=np.zeros((3, sim.nq + 1), np.float32))), (("left", tp), dict(damping=0.0)), (("left", tp), dict(max_step=-1.0)),
                     (("left", tp), dict(tol=-1.0)), (("left", tp), dict(max_iters=-1)), (("left", tp), dict(dofs=np.ones(sim.nv + 1, bool))), (("left", tp), dict(mask=np.ones(4))),
                     (((), tp), {}), ((("left",) * 5, np.zeros((3, 5, 3), np.float32)), {}), (("left", tp), dict(out=(tp, tp, tp)))):
        with pytest.raises(ValueError):
            sim.solve_ik(*args, **kw)
    with pytest.raises(KeyError):
        sim.solve_ik("nowhere", tp)
    assert sim._t is None, "nothing touched the device"


@pytest.mark.parametrize("name", list(I.XML))
def test_the_reference_reaches_its_targets(name):
    """the condition on the cases (the seed of ik_cases.case is chosen so that it holds): the fp64 reference converges in at most max_iters / 2 updates in every world"""
    _, err, iters = I.reference(name)
    assert (err < I.KW["tol"]).all() and (iters <= I.KW["max_iters"] // 2).all(), (err, iters)
