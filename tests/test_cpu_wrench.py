"""The body-wrench block of grx.BatchedSim without a device: body_dynamics= validation and shapes, the force / torque sensor rows, and the yardstick of tests/test_gpu_wrench.py
itself -- two closed forms of tests/wrench_refs.py, and its own error estimate below a tenth of every bound for every world and case compared on the GPU."""
import json
import os

import numpy as np
import pytest

import dyn_tree_cases as D
import engine_matrix_cases as C
import sensor_cases as SC
import wrench_refs as WR
from test_cpu_sensors import acc_bound

import gymnasium_robotics_amd as grx
from gymnasium_robotics_amd import sim as simmod

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrench_errors.json")
RUNS = [("hinge-arm", 5), ("free-tree", 5), ("free-v0", 5), ("free-v7", 5), ("deep", 5), ("free-tree", 13)]
_REF = {}


def force_bound():
    """twice the worst force figure of the MI355X over the tree cases (tests/golden/wrench_errors.json, written by tools/wrench_errors.py)"""
    with open(GOLDEN) as fh:
        return 2.0 * max(json.load(fh)["device"].values())


def rows_of(model):
    return [name for name, _ in sorted(model.names["body"].items(), key=lambda kv: kv[1])]


def applied_of(case):
    """a non-zero xfrc_applied (f, t) on one mid-tree row and one leaf row of the compiled model (the last row is a leaf; a model with one body has both on it, the later entry)"""
    rows = rows_of(case.model)
    return {rows[max(1, (len(rows) - 1) // 2)]: (np.array([1.5, -2.0, 4.0]), np.array([0.3, 0.2, -0.4])), rows[-1]: (np.array([-0.5, 0.25, 1.0]), np.array([-0.1, 0.05, 0.2]))}


def reference(name, n):
    """per world the dict of wrench_refs.evaluate; computed once, read only"""
    if (name, n) not in _REF:
        case, st = SC.CASES[name], SC.CASES[name].states(n)
        _REF[(name, n)] = [WR.evaluate(case.tree, st["qpos"][i], st["qvel"][i], rows_of(case.model), applied_of(case)) for i in range(n)]
    return _REF[(name, n)]


def force_scale(case, ref, key):
    return 1.0 + ref["mass"] * float(np.linalg.norm(case.tree["gravity"])) + float(np.abs(ref[key]).max())


def test_validation_shapes_and_sensor_rows():
    case = SC.CASES["hinge-arm"]
    assert simmod.BODY_DYNAMICS == ("cfrc_ext", "cfrc_int", "cacc", "subtree_com") and simmod.SENSOR_TYPES[-2:] == ("force", "torque") and simmod.SENSOR_TYPES.index("accelerometer") == 17
    sim = grx.BatchedSim(case.model, 3, body_dynamics=("subtree_com", "cfrc_int"))
    assert sim.body_dynamics == ("cfrc_int", "subtree_com") and sim._shapes()["cfrc_int"] == (3, sim.nbody, 6) and sim._shapes()["subtree_com"] == (3, sim.nbody, 3)
    with pytest.raises(AttributeError, match="body_dynamics"):
        sim.cacc
    for bad, why in ((("cfrc",), "unknown body_dynamics"), (("cacc", "cacc"), "twice")):
        with pytest.raises(ValueError, match=why):
            grx.BatchedSim(case.model, 3, body_dynamics=bad)
    xml = case.xml.replace("</sensor>", '<force name="ft_f" site="tip" cutoff="2.5"/><torque name="ft_t" site="tip"/><force name="on_body" body="h1"/></sensor>')
    sim = grx.BatchedSim(C.compile_xml(xml), 3, sensors=("ft_f", "ft_t"), body_dynamics=("cfrc_int",))
    T, tip = simmod.SENSOR_TYPES.index, sim.site_id("tip")
    assert sim._sensor_spec == [(T("force"), 2, tip, 0), (T("torque"), 2, tip, 3)] and sim._sensor_cut == [2.5, 0.0] and sim.nsensordata == 6
    for kw, name, why in ((dict(body_dynamics=("cfrc_int",)), "on_body", "attached to a site"), ({}, "ft_f", "name 'cfrc_int' in body_dynamics")):
        with pytest.raises(ValueError, match=why):
            grx.BatchedSim(C.compile_xml(xml), 3, sensors=(name,), **kw)
        assert why in grx.BatchedSim(C.compile_xml(xml), 3, sensors="all", **kw).sensors_unserved[name]


def test_reference_closed_forms():
    """a hinge body at rest is held by m g up at its joint (the axis along gravity: no torque about it wherever the centre of mass is); nothing holds a free body"""
    gravity = SC.CASES["hinge-arm"].tree["gravity"]
    hang = D.Case("hang", 1, [D.B("p", None, pos=(0.1, 0.2, 1.0), joints=[D.J("hinge", "pj", axis=tuple(gravity))], inertial=dict(mass=2.0, pos=(0.1, 0.0, -0.3), diag=[0.01, 0.02, 0.03]))])
    tree = hang.tree
    m, g = tree["bodies"][0]["mass"], np.asarray(tree["gravity"], dtype=np.float64)
    ref = WR.evaluate(tree, np.zeros(1), np.zeros(1), ["world", "p"])
    print("hanging body", ref["cfrc_int"][1], "m g", m * g)
    assert np.abs(ref["cfrc_int"][1, 3:] + m * g).max() <= 1e-9 * m * np.linalg.norm(g) and np.abs(ref["cacc"][1] - ref["cacc"][0]).max() <= 1e-9
    free, st = SC.CASES["free-v7"], SC.CASES["free-v7"].states(1)
    ref = WR.evaluate(free.tree, st["qpos"][0], st["qvel"][0], rows_of(free.model))
    assert np.abs(ref["cfrc_int"][1]).max() <= 1e-7 * force_scale(free, ref, "cfrc_int")


@pytest.mark.parametrize("name,n", RUNS)
def test_reference_error_is_below_a_tenth_of_the_bound(name, n):
    case = SC.CASES[name]
    assert force_bound() <= SC.ACC_MAX and acc_bound() <= SC.ACC_MAX
    for ref in reference(name, n):
        g = float(np.linalg.norm(case.tree["gravity"]))
        figs = dict(cfrc_int=ref["err"]["cfrc_int"].max() / force_scale(case, ref, "cfrc_int") / force_bound(), cfrc_ext=ref["err"]["cfrc_ext"] / force_scale(case, ref, "cfrc_ext") / force_bound(),
                    cacc=ref["err"]["cacc"].max() / (1.0 + g + np.abs(ref["cacc"]).max()) / acc_bound(), subtree_com=ref["err"]["subtree_com"] / C.BOUND)
        assert max(figs.values()) <= 0.1, figs
