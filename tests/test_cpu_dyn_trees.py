"""The compiler, the fp64 oracle and the lane emulator against tests/dyn_refs.py on the trees of tests/dyn_tree_cases.py -- the first half of every forward pass, held to a
reference that shares neither the compiler's tables nor the oracle's recursion.

(a) the compiled tables against the description: masses, centres of mass, inertia tensors, joint axes and anchors, qpos0, the passive parameters;
(b) OracleSim.forward() and step(1) field by field: the bound is 10 x the reference's own error estimate and never above 1e-6 max(1, |value|), two orders below what the
    device is held to, so reference error cannot pay for a device error;
(c) the emulator within the project's 1e-4 on qpos', qvel', xpos, xmat and qM, and -- it is the device's source in fp32 -- within the device's vector bounds on qfrc_smooth
    (= qfrc_passive - qfrc_bias here) and qacc_smooth, which outlive the step in its working set (qfrc_bias itself is overlaid by the solve);
(d) the preconditions of the device comparison, on the reference alone, no case or world left out: no field of any world moves by SENS_MAX under a one-ulp jitter of the
    fp32 start (tests/test_cpu_sim_dynamics.py), and merely STORING the inputs of qfrc_bias and of the solve for qacc_smooth in fp32 moves neither by as much as the bound the
    device is held to (dyn_tree_cases.fp32_conditioning: below that, a failure is the engine's and not the number format's).
tests/golden/dyn_tree_errors.json (tools/measure_dyn_trees.py) records the worst figures; they are a record, no bound here comes from them."""
import json
import math
import os
import types

import numpy as np
import pytest

import dyn_refs as R
import dyn_tree_cases as T
import engine_matrix_cases as C

CEILING = 1e-6


# (a) -------------------------------------------------------------------------------------------------------------------------------------------------------
def _rest_in_carrier(case):
    """{body: (carrier, pos, rotation)}: the pose of every body in the frame of the body that carries it, from the description (joint-less bodies only chain fixed poses)"""
    by = {b["name"]: b for b in case.tree["bodies"]}
    names = [b["name"] for b in case.tree["bodies"]]
    out = {}
    for name in names:
        b = by[name]
        if b["joints"]:
            out[name] = (name, np.zeros(3), np.eye(3))
        elif b["parent"] < 0:
            out[name] = (None, np.asarray(b["pos"]), R.qmat(R.unit(b["quat"])))
        else:
            car, p, Rm = out[names[b["parent"]]]
            out[name] = (car, p + Rm @ np.asarray(b["pos"]), Rm @ R.qmat(R.unit(b["quat"])))
    return out


@pytest.mark.parametrize("name", T.NAMES)
def test_compiled_tables_equal_the_description(name):
    case = T.CASES[name]
    m, tree = case.model, case.tree
    t, rows = m.tables, m.names["body"]
    T.joint_layout_matches(case)
    by = {b["name"]: b for b in tree["bodies"]}
    rest = _rest_in_carrier(case)
    assert set(rows) == set(case.moving) | {"world"}
    assert abs(np.asarray(t["body_mass"]).sum() - sum(b["mass"] for b in tree["bodies"])) < 1e-12
    worst = dict(mass=0.0, ipos=0.0, inertia=0.0)
    for car in case.moving:
        parts = []
        for b, (c, p, Rm) in rest.items():
            if c == car:
                parts.append((by[b]["mass"], p + Rm @ np.asarray(by[b]["ipos"]), Rm @ np.asarray(by[b]["inertia"]) @ Rm.T))
        mass, com, I = T.combine(parts)
        k = rows[car]
        f = np.asarray(t["body_inertia"]).reshape(-1, 6)[k]      # the full tensor about body_ipos in the body's frame (the compiled model carries no principal frame)
        full = np.array([[f[0], f[3], f[4]], [f[3], f[1], f[5]], [f[4], f[5], f[2]]])
        worst["mass"] = max(worst["mass"], abs(np.asarray(t["body_mass"]).reshape(-1)[k] - mass))
        worst["ipos"] = max(worst["ipos"], np.abs(np.asarray(t["body_ipos"]).reshape(-1, 3)[k] - com).max())
        worst["inertia"] = max(worst["inertia"], np.abs(full - I).max() / np.abs(I).max())
        assert np.all(np.linalg.eigvalsh(full) > 0)
    lay = R.layout(tree)[0]
    for k, (b, j, qa, da) in enumerate(lay):
        jt = tree["bodies"][b]["joints"][j]
        assert int(np.asarray(t["jnt_bodyid"]).reshape(-1)[k]) == rows[tree["bodies"][b]["name"]]
        assert int(np.asarray(t["jnt_type"]).reshape(-1)[k]) == {"free": 0, "slide": 2, "hinge": 3}[jt["type"]]
        if jt["type"] == "free":
            continue
        assert np.abs(np.asarray(t["jnt_axis"]).reshape(-1, 3)[k] - jt["axis"]).max() < 1e-15 and np.abs(np.asarray(t["jnt_pos"]).reshape(-1, 3)[k] - jt["pos"]).max() < 1e-15, jt["name"]
        for table, key, idx in (("dof_armature", "armature", da), ("dof_damping", "damping", da), ("jnt_stiffness", "stiffness", k), ("jnt_springref", "springref", k)):
            assert abs(np.asarray(t[table]).reshape(-1)[idx] - jt[key]) < 1e-15, (jt["name"], table)
    q0 = R.qpos0(tree)
    d0 = np.abs(np.asarray(t["qpos0"]).reshape(-1) - q0).max()
    print(name, "mass", worst["mass"], "ipos", worst["ipos"], "inertia (relative)", worst["inertia"], "qpos0", d0)
    assert worst["mass"] < 1e-14 and worst["ipos"] < 1e-15 * 64 and worst["inertia"] < 1e-13 and d0 < 1e-14
    assert abs(m.opt("timestep") - T.TIMESTEP) == 0 and [m.opt("gravity_" + a) for a in "xyz"] == list(T.GRAVITY)
    assert m.dim("nu") == 0 and m.dim("ngeom") == 0 and m.dim("npair") == 0 and m.dim("integrator") == 0


def test_cases_are_what_they_are_for():
    for name, case in T.CASES.items():
        tree = case.tree
        moving_depth = {b["name"]: sum(1 for a in np.nonzero(R.ancestors(tree)[k])[0] if tree["bodies"][a]["joints"]) for k, b in enumerate(tree["bodies"])}
        sited = [b for b in tree["bodies"] if b["sites"]]
        deepest = max(moving_depth[b["name"]] for b in tree["bodies"] if b["joints"])
        assert any(b["joints"] and moving_depth[b["name"]] == deepest for b in sited), name      # a site on a deepest leaf
        assert any(not b["joints"] for b in sited), name                                            # and one on a joint-less child
        assert 2 <= len(case.site_names) <= 16
    xml = T.CASES["spellings"].xml
    assert all(f' {k}="' in xml for k in ("euler", "axisangle", "xyaxes", "zaxis", "quat")) and 'eulerseq="zyx"' in xml and 'angle="degree"' in xml
    assert all(j["ref"] != 0 and np.abs(j["pos"]).max() > 0 for b in T.CASES["spellings"].bodies for j in b["joints"])
    kinds = lambda n: [[j["type"] for j in b["joints"]] for b in T.CASES[n].bodies]
    assert ["slide", "slide", "hinge"] in kinds("multi-joint") and ["hinge", "hinge"] in kinds("multi-joint")
    assert "fullinertia" in T.CASES["inertial"].xml and "diaginertia" in T.CASES["inertial"].xml
    for b in T.CASES["inertial"].tree["bodies"]:      # principal axes far from the body axes
        if b["joints"]:
            assert np.abs(b["inertia"] - np.diag(np.diag(b["inertia"]))).max() > 0.1 * np.abs(np.diag(b["inertia"])).min()
    dx = T.CASES["density"].xml
    assert all(f'type="{k}"' in dx for k in ("sphere", "capsule", "cylinder", "ellipsoid", "box")) and "fromto" in dx and ' mass="' in dx
    assert any(len(b["geoms"]) == 2 for b in T.CASES["density"].bodies)
    fc = {b["name"]: b for b in T.CASES["fixed-children"].bodies}
    assert not fc["f0a"]["joints"] and not fc["f0b"]["joints"] and fc["f0b"]["parent"] == "f0a" and fc["f1"]["parent"] == "f0b"      # two deep, carrying a jointed child
    df = T.CASES["defaults"].xml
    assert "childclass" in df and df.count("<default") == 3 and df.count("stiffness") == 1 and 'class="wrist"' in df
    assert [R.layout(T.CASES[f"depth-{n}"].tree)[2] for n in (2, 3, 5, 9, 17)] == [2, 3, 5, 9, 17]
    assert [T.CASES[f"depth-{n}"].model.dim("maxdepth") for n in (2, 3, 5, 9, 17)] == [2, 3, 5, 9, 17]      # one past a power of two each
    assert T.CASES["wide"].model.dim("nbody") == 22 and T.CASES["wide"].model.dim("maxdepth") == 2
    assert T.CASES["two-trees"].model.dim("ntree") == 3
    M = T.reference("two-trees", T.N_WORLDS)["M"]
    blocks = np.zeros((10, 10), dtype=bool)
    for a, b in ((0, 6), (6, 9), (9, 10)):
        blocks[a:b, a:b] = True
    assert not M[:, ~blocks].any() and (np.abs(M[:, 6:9, 6:9]) > 0).all()
    for name in ("free-root-alone", "free-root-tree", "two-trees"):
        st = T.CASES[name].states(T.N_WORLDS)
        assert (np.abs(st["qpos"][1:, 3]) <= 0.7 + 1e-6).all()      # far from the identity
    for name in ("free-root-alone", "free-root-tree"):
        st = T.CASES[name].states(T.N_WORLDS)
        assert np.allclose(np.linalg.norm(st["qvel"][1:, 3:6], axis=1), 10.0, atol=1e-5)
        b = T.CASES[name].tree["bodies"][0]
        assert np.abs(b["ipos"]).min() > 0.03 and np.abs(b["inertia"] - np.diag(np.diag(b["inertia"]))).max() > 1e-3
    for name, case in T.CASES.items():
        st = case.states(T.N_WORLDS)
        assert not st["qvel"][0].any() and np.array_equal(st["qpos"][0], R.qpos0(case.tree).astype(np.float32).astype(np.float64))
        assert np.array_equal(case.states(13)["qpos"][:T.N_WORLDS], st["qpos"]) and np.array_equal(st["qpos"], st["qpos"].astype(np.float32))


def test_full_is_at_the_compilers_limits():
    """`full` has as many moving bodies as the compiler admits: one more is refused by the compiler's own check.  Its 64 dofs are the engine's limit, which the model
    handle checks on the device (tests/test_gpu_dyn_trees.py)."""
    case = T.CASES["full"]
    assert case.model.dim("nbody") == T.MAX_BODIES + 1 and case.model.dim("nv") == T.MAX_DOFS == R.layout(case.tree)[2]
    rng = np.random.default_rng(1)
    more = T.Case("one-more", 99, list(case.bodies) + [T._rand_link(rng, "extra", "b3", "hinge")])
    with pytest.raises(ValueError, match="at most 64 bodies"):
        more.model


# (b) -------------------------------------------------------------------------------------------------------------------------------------------------------
def compare_oracle(name, n):
    """{field: (worst error, worst error / bound, worst estimate)} of the oracle against the reference, bound = min(10 x estimate, CEILING max(1, |value|)) per element"""
    want, err = T.want(name, n)
    got = dict(T.oracle_run(name, n))
    got["xquat"] = R.sign_like(got["xquat"], want["xquat"])
    out = {}
    for k in T.FORWARD_FIELDS + T.STEP_FIELDS + ("site_xvelp", "site_xvelr"):
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        d = np.abs(got[k] - want[k])
        bound = np.minimum(10.0 * err[k], CEILING * np.maximum(1.0, np.abs(want[k])))
        ratio = np.where(d <= bound, np.divide(d, bound, out=np.zeros_like(d), where=bound > 0), np.inf)
        out[k] = (float(d.max(initial=0.0)), float(ratio.max(initial=0.0)), float(np.max(err[k], initial=0.0)))
    assert not got["qfrc_constraint"].any()
    return out


@pytest.mark.parametrize("name,n", T.RUNS)
def test_oracle_equals_the_reference(name, n):
    fig = compare_oracle(name, n)
    print(name, n, "oracle vs reference, error (share of its bound):", " ".join(f"{k} {v[0]:.1e} ({v[1]:.2f})" for k, v in fig.items()))
    assert all(v[1] <= 1.0 for v in fig.values()), {k: v for k, v in fig.items() if not v[1] <= 1.0}


# (c) -------------------------------------------------------------------------------------------------------------------------------------------------------
def emulate(name, n):
    """{field: worst absolute error over the n worlds} of the emulator's step(1) against the reference"""
    from emu_sim import EmuSim

    case = T.CASES[name]
    m, st = case.model, case.states(n)
    want, _ = T.want(name, n)
    emu = EmuSim(m, types.SimpleNamespace(obs_dim=1))
    nb, nv = m.dim("nbody"), m.dim("nv")
    import sim_dyn_cases as D

    worst = dict(qpos1=0.0, qvel1=0.0, xpos=0.0, xmat=0.0, qM=0.0, qfrc_smooth=0.0, qacc_smooth=0.0)
    for i in range(n):
        emu.qpos[:], emu.qvel[:], emu.qacc_ws[:] = st["qpos"][i], st["qvel"][i], 0.0
        ncon, nefc = emu.physics_steps(1)
        assert emu.status.value == 0 and (ncon, nefc) == (0, 0), (name, i, emu.status.value, ncon, nefc)
        got = dict(qpos1=emu.qpos.copy(), qvel1=emu.qvel.copy(), xpos=emu.ctx("xpos", 3 * nb).reshape(nb, 3), xmat=emu.ctx("xmat", 9 * nb).reshape(nb, 9), qM=emu.ctx("M", nv * nv).reshape(nv, nv))
        ref = dict(qpos1=want["qpos1"][i], qvel1=want["qvel1"][i], xpos=want["xpos"][i], xmat=np.stack([R.qmat(q).reshape(9) for q in want["xquat"][i]]), qM=want["M"][i])
        for k in got:
            d = np.abs(got[k].astype(np.float64) - ref[k]).max()
            worst[k] = max(worst[k], float(d) if np.isfinite(d) else np.inf)
        for k in ("qfrc_smooth", "qacc_smooth"):      # of the step's forward pass, in the measure the device is held to
            worst[k] = max(worst[k], float(D.error(k, emu.ctx(k, nv)[None], want[k][i][None])[0]))
    return worst


@pytest.mark.parametrize("name,n", T.RUNS)
def test_emulator_equals_the_reference(name, n):
    worst = emulate(name, n)
    print(name, n, "emulator vs reference:", " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    bound = _vector_bounds()
    assert all(v < C.BOUND for v in worst.values()) and all(worst[k] <= bound[k] for k in ("qfrc_smooth", "qacc_smooth")), (worst, bound)


# (d) -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", T.RUNS)
def test_every_world_is_well_posed_for_the_reference(name, n):
    assert T.DRAWS == C.DRAWS
    sens = T.reference_sensitivity(name, n)
    worst = {k: float(v.max()) for k, v in sens.items()}
    print(name, n, "reference sensitivity:", " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(v < C.SENS_MAX for v in worst.values()), {k: [(i, float(s)) for i, s in enumerate(v) if not s < C.SENS_MAX] for k, v in sens.items() if not (v < C.SENS_MAX).all()}


def _vector_bounds():
    """the bounds the device's vectors are held to (tests/test_gpu_sim_dynamics.py::vector_bounds, read here without importing a GPU test module's dependencies)"""
    import sim_dyn_cases as D

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim_dynamics_errors.json")) as fh:
        table = json.load(fh)["worst_error"]
    rows = [f"{s}/{k}/5" for s, k in D.CASES if s in D.BOUND_SCENES] + ["arm/1/13"]
    return {f: 10.0 ** math.ceil(math.log10(4.0 * max(table[c][f] for c in rows))) for f in ("qfrc_bias", "qfrc_smooth", "qacc_smooth")}


@pytest.mark.parametrize("name,n", T.RUNS)
def test_fp32_storage_alone_stays_inside_the_device_bounds(name, n):
    cond, bound = T.fp32_conditioning(name, n), _vector_bounds()
    worst = {k: float(v.max()) for k, v in cond.items()}
    print(name, n, "fp32 storage conditioning:", " ".join(f"{k} {v:.1e} (bound {bound[k]:.0e})" for k, v in worst.items()))
    assert all(worst[k] < bound[k] for k in worst), (worst, bound)
