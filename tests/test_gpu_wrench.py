"""The body-wrench block of grx.BatchedSim on the GPU (pytest -m gpu): subtree_com, cfrc_ext, cacc and cfrc_int against the fp64 reference (tests/wrench_refs.py) on tree cases
of tests/sensor_cases.py, cfrc_ext against the contact outputs of the same launch, the force / torque sensors against their definition, and the plumbing.  N = 5 worlds per
case, 13 once; every requested row starts as NaN.  The reference's own error is asserted below a tenth of every bound in tests/test_cpu_wrench.py.

Bounds: subtree_com engine_matrix_cases.BOUND absolute; force-type rows |got - want|_inf / (1 + sum_b m_b |g| + max_b |want_b|_inf) per world, against twice the worst such
figure measured on the MI355X over the tree cases (tests/golden/wrench_errors.json, tools/wrench_errors.py), which may not exceed 1e-3; cacc the sensor tests' acceleration
rule.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import engine_matrix_cases as C
import sensor_cases as SC
import sim_cases as S
from test_cpu_sensors import acc_bound
from test_cpu_wrench import RUNS, applied_of, force_bound, force_scale, reference
from test_gpu_sensors import _resting, host

pytestmark = pytest.mark.gpu
N, G = 5, 9.81
ALL = ("cfrc_ext", "cfrc_int", "cacc", "subtree_com")
FT = '<force name="ft_f" site="{0}"/><torque name="ft_t" site="{0}"/><force name="ft_cut" site="{0}" cutoff="0.05"/></sensor>'
ARM_FT, RK4_FT, HINGE_FT = SC.ARM_XML.replace("</sensor>", FT.format("pad")), SC.RK4_XML.replace("</sensor>", FT.format("tip")), SC.CASES["hinge-arm"].xml.replace("</sensor>", FT.format("tip"))


def make(model, n, st, **kw):
    import torch

    import gymnasium_robotics_amd as grx

    sim = grx.BatchedSim(model, n, **kw)
    for k, v in st.items():
        getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).reshape(getattr(sim, k).shape))
    for k in sim.body_dynamics + (("sensor_data",) if sim.sensors else ()):
        getattr(sim, k).fill_(float("nan"))
    return sim


ARM_SITES = SC.ARM_XML.replace('<body name="link3" pos="0.2 0 0">', '<site name="s2"/><body name="link3" pos="0.2 0 0"><site name="s3"/>').replace('<body name="link2" pos="0 0 0.2">', '<site name="s1"/><body name="link2" pos="0 0 0.2">')
_SCENES = {"arm_ft": SC.SensorScene("arm_ft", "arm", ARM_FT), "rk4_ft": SC.SensorScene("rk4_ft", "rk4", RK4_FT),
           "arm_sites": S.Scene("arm", ARM_SITES, 11, compile_kwargs=dict(touch_filter=lambda name: True, keep_sites=("ee", "pad", "s1", "s2", "s3")))}


def scene(name, n=N, st=None, **kw):
    sc = _SCENES.get(name) or SC.SCENES[name]
    return make(sc.model, n, sc.states(n) if st is None else st, **kw)


def rows(sim, keys=ALL):
    return {k: host(getattr(sim, k)).astype(np.float64) for k in keys}


_ROWS = {}


def tree_rows(name, n):
    import torch

    if (name, n) not in _ROWS:
        case = SC.CASES[name]
        sim = make(case.model, n, case.states(n), body_dynamics=ALL, applied=("xfrc_applied",))
        for row, (f, t) in applied_of(case).items():
            sim.xfrc_applied[:, sim.body_id(row)] = torch.tensor(np.concatenate([f, t]), dtype=torch.float32, device=sim.device)
        sim.forward()
        _ROWS[(name, n)] = rows(sim)
        sim.close()
    return _ROWS[(name, n)]


def figures(name, n):
    """per output the worst figure over the case's worlds: subtree_com absolute, the force rows and cacc relative to their scales (module docstring)"""
    case, got, g = SC.CASES[name], tree_rows(name, n), float(np.linalg.norm(SC.CASES[name].tree["gravity"]))
    out = dict.fromkeys(ALL, 0.0)
    for i, ref in enumerate(reference(name, n)):
        scale = dict(subtree_com=1.0, cacc=1.0 + g + np.abs(ref["cacc"]).max(), cfrc_int=force_scale(case, ref, "cfrc_int"), cfrc_ext=force_scale(case, ref, "cfrc_ext"))
        for k in ALL:
            assert np.isfinite(got[k][i]).all(), (k, i)
            out[k] = max(out[k], float(np.abs(got[k][i] - ref[k]).max() / scale[k]))
    return out


@pytest.mark.parametrize("name,n", RUNS)
def test_trees_match_the_reference(name, n):
    fig = figures(name, n)
    print(name, n, fig, "bounds", C.BOUND, force_bound(), acc_bound())
    assert force_bound() <= SC.ACC_MAX
    assert fig["subtree_com"] <= C.BOUND and fig["cfrc_int"] <= force_bound() and fig["cfrc_ext"] <= force_bound() and fig["cacc"] <= acc_bound()
    if name == "free-v7":      # a boost of the free root changes no force, and the spatial acceleration by what the reference says
        a, b, ra, rb, case = tree_rows("free-v0", n), tree_rows(name, n), reference("free-v0", n), reference(name, n), SC.CASES[name]
        for i in range(n):
            for k in ("cfrc_int", "cfrc_ext"):
                assert np.abs(a[k][i] - b[k][i]).max() <= force_bound() * force_scale(case, rb[i], k)
            d, want = b["cacc"][i] - a["cacc"][i], rb[i]["cacc"] - ra[i]["cacc"]
            assert (i == 0 or np.abs(want).max() > 1.0) and np.abs(d - want).max() <= acc_bound() * (1.0 + G + np.abs(rb[i]["cacc"]).max())      # (world 0 does not rotate)


@pytest.mark.parametrize("per_world", [False, True])
def test_free_root_carries_no_load(per_world):
    import torch

    sc = SC.SCENES["arm"]
    sim = scene("arm", st=_resting(sc.states(N), N), body_dynamics=ALL, model_params=("gravity", "body_mass") if per_world else ())
    box, mass, g = sim.body_id("box"), np.full(N, 0.1), np.full(N, G)
    if per_world:
        mass, g = 0.1 * np.array([0.5, 0.75, 1.0, 1.5, 2.0]), G * np.array([1.2, 1.1, 1.0, 0.9, 0.8])
        sim.params.body_mass[:, box] = torch.from_numpy(mass.astype(np.float32)).to(sim.device)
        sim.params.gravity[:, 2] = torch.from_numpy(-g.astype(np.float32)).to(sim.device)
        sim.commit_params()
    sim.step(500)
    r = rows(sim)
    scale = 1.0 + (1.4 + mass) * g + np.abs(r["cfrc_ext"][:, box]).max(axis=1)      # (the arm weighs 1.4 kg)
    fig = dict(cfrc_int=np.abs(r["cfrc_int"][:, box]).max(axis=1) / scale, weight=np.abs(r["cfrc_ext"][:, box, 3:] - np.stack([0 * g, 0 * g, mass * g], axis=1)).max(axis=1) / scale,
               reaction=np.abs(r["cfrc_ext"][:, 0, 3:] + r["cfrc_ext"][:, box, 3:]).max(axis=1) / scale)
    print("resting box", r["cfrc_ext"][:, box], fig)
    assert all((v <= force_bound()).all() for v in fig.values())
    sim.close()


@pytest.mark.parametrize("name", ["arm", "pile"])
def test_cfrc_ext_equals_the_contact_outputs_of_the_same_launch(name):
    sim = scene(name, body_dynamics=("cfrc_ext", "subtree_com"), contacts=("contact_geom", "contact_pos", "contact_frame", "contact_force"), applied=("xfrc_applied", "xipos"), outputs=("ncon",))
    sim.xfrc_applied[:, sim.nbody - 1] = 0.25
    sim.step(3)
    r, tb = rows(sim, ("cfrc_ext", "subtree_com", "contact_pos", "contact_frame", "contact_force", "xfrc_applied", "xipos")), sim.model.tables
    geom, ncon, gb, root, mass = host(sim.contact_geom), host(sim.ncon), *(np.asarray(tb[k]).reshape(-1) for k in ("geom_bodyid", "body_rootid", "body_mass"))
    if name == "pile":
        print("ncon", ncon)
        assert (ncon[1:] > S.PILE_MAXCON).all() and np.isfinite(r["cfrc_ext"]).all()      # worlds 1 .. 4 ran again on the large tables
    for w in range(N):
        want, com = np.zeros((sim.nbody, 6)), r["subtree_com"][w][root]
        for b in range(1, sim.nbody):
            f, t = r["xfrc_applied"][w, b, :3], r["xfrc_applied"][w, b, 3:]
            want[b] = np.concatenate([t + np.cross(r["xipos"][w, b] - com[b], f), f])
        for k in range(ncon[w]):
            fr, cf = r["contact_frame"][w, k].reshape(3, 3), r["contact_force"][w, k]
            for b, s in ((gb[geom[w, k, 0]], -1.0), (gb[geom[w, k, 1]], 1.0)):
                want[b] += s * np.concatenate([fr.T @ cf[3:] + np.cross(r["contact_pos"][w, k] - com[b], fr.T @ cf[:3]), fr.T @ cf[:3]])
        fig = np.abs(r["cfrc_ext"][w] - want).max() / (1.0 + mass.sum() * G + np.abs(want).max())
        print(name, w, "contacts", ncon[w], "figure", fig)
        assert fig <= force_bound()
    assert np.abs(r["cfrc_ext"][:, 0]).max() > 0.1      # the floor's reactions are on the world's row
    sim.close()


@pytest.mark.parametrize("dof", range(4))
def test_cfrc_int_projects_onto_the_joint(dof):
    """a hinge whose limit is inactive transmits passive + actuator + applied along its axis, less what its armature takes (armature qacc: rotor inertia is no part of any
    body's cinert, in MuJoCo as here): the site Jacobian column of the dof against cfrc_int of the dof's body"""
    names = ("link1", "link2", "link3", "link4")
    st = {k: v.copy() for k, v in SC.SCENES["arm"].states(N).items()}
    st["qpos"][:, :4] *= 0.25      # away from every joint limit
    sim = scene("arm_sites", st=st, body_dynamics=("cfrc_int", "subtree_com"), outputs=("site_xpos", "site_jacp", "site_jacr", "qfrc_passive", "qfrc_actuator", "qacc"), jac_sites=("s1", "s2", "s3", "ee"), applied=("qfrc_applied",))
    sim.qfrc_applied[:, :4] = 0.125
    sim.forward()
    site = ("s1", "s2", "s3", "ee")[dof]
    b, r = sim.body_id(names[dof]), rows(sim, ("cfrc_int", "subtree_com", "site_xpos", "site_jacp", "site_jacr", "qfrc_passive", "qfrc_actuator", "qacc"))
    tau, f, c = r["cfrc_int"][:, b, :3], r["cfrc_int"][:, b, 3:], r["subtree_com"][:, sim.body_id("link1")]
    p, jp, jr = r["site_xpos"][:, sim.site_id(site)], r["site_jacp"][:, sim.jac_row(site), :, dof], r["site_jacr"][:, sim.jac_row(site), :, dof]
    got = np.einsum("nk,nk->n", jr, tau - np.cross(p - c, f)) + np.einsum("nk,nk->n", jp, f)
    want = r["qfrc_passive"][:, dof] + r["qfrc_actuator"][:, dof] + 0.125 - float(np.asarray(sim.model.tables["dof_armature"]).reshape(-1)[dof]) * r["qacc"][:, dof]
    fig = np.abs(got - want) / (1.0 + 1.5 * G + np.abs(r["cfrc_int"][:, b]).max(axis=1))
    print("dof", dof, got, want, fig)
    assert (fig <= force_bound()).all()
    sim.close()


def _definition(sim, site, r, cut=0.05):
    b, s = int(np.asarray(sim.model.tables["site_bodyid"]).reshape(-1)[sim.site_id(site)]), sim.site_id(site)
    root = int(np.asarray(sim.model.tables["body_rootid"]).reshape(-1)[b])
    tau, f, c, p, Rm = r["cfrc_int"][:, b, :3], r["cfrc_int"][:, b, 3:], r["subtree_com"][:, root], r["site_xpos"][:, s], r["site_xmat"][:, s].reshape(-1, 3, 3)
    force, torque = np.einsum("nji,nj->ni", Rm, f), np.einsum("nji,nj->ni", Rm, tau - np.cross(p - c, f))
    return np.concatenate([force, torque, np.clip(force, -cut, cut)], axis=1), 1.0 + np.abs(r["cfrc_int"][:, b]).max(axis=1, keepdims=True)


FT_KW = dict(sensors=("ft_f", "ft_t", "ft_cut"), body_dynamics=("cfrc_int", "subtree_com"), outputs=("site_xpos", "site_xmat"))


@pytest.mark.parametrize("name,site", [("hinge-arm", "tip"), ("arm_ft", "pad")])
def test_force_and_torque_sensors_are_their_definition(name, site):
    sim = make(C.compile_xml(HINGE_FT), N, SC.CASES[name].states(N), **FT_KW) if name in SC.CASES else scene(name, **FT_KW)
    sim.forward()
    want, scale = _definition(sim, site, rows(sim, ("cfrc_int", "subtree_com", "site_xpos", "site_xmat")))
    got = host(sim.sensor_data).astype(np.float64)
    print(site, "force / torque", got[0], "figure", (np.abs(got - want) / scale).max())
    assert (np.abs(got - want) <= force_bound() * scale).all()
    cut = float(np.float32(0.05))
    assert ((np.abs(got[:, :3]) > cut).any() or site == "pad") and (got[:, 6:] == np.clip(got[:, :3], -cut, cut)).all()      # the cutoff bites on the arm (the free box carries no load)
    sim.close()


def test_rk4_sensors_read_the_first_stage_cfrc_int_the_fourth():
    a, b = scene("rk4_ft", **FT_KW), scene("rk4_ft", **FT_KW)
    a.step(1)
    b.forward()
    got, start, qvel = host(a.sensor_data).astype(np.float64), host(b.sensor_data).astype(np.float64), host(b.qvel)
    fourth, _ = _definition(a, "tip", rows(a, ("cfrc_int", "subtree_com", "site_xpos", "site_xmat")))
    bound = C.BOUND * (1.0 + np.abs(qvel).sum(axis=1, keepdims=True))      # the velocity bound of tests/test_gpu_sensors.py
    print("vs forward() at the start", (np.abs(got - start) / bound).max(), "vs the fourth stage", (np.abs(got - fourth)[:, :6].max(axis=1, keepdims=True) / bound).ravel())
    assert (np.abs(got - start) <= bound).all() and (np.abs(got - fourth)[:, :6].max(axis=1, keepdims=True) > bound).all()
    a.close(), b.close()


def test_step_is_step_and_forward_and_masked_worlds_keep_their_bits():
    import torch

    kw = dict(sensors=("ft_f", "ft_t"), body_dynamics=ALL)
    a, b = scene("arm_ft", **kw), scene("arm_ft", **kw)
    a.step(3)
    b.step(2)
    for k in ALL + ("sensor_data",):
        getattr(b, k).fill_(float("nan"))
    b.forward()
    assert all(host(getattr(a, k)).tobytes() == host(getattr(b, k)).tobytes() for k in ALL + ("sensor_data",))
    keep = {k: host(getattr(b, k).fill_(-7.5)) for k in ALL + ("sensor_data",)}
    b.step(1, mask=torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8, device=b.device))
    for k in ALL + ("sensor_data",):
        got = host(getattr(b, k))
        assert got[[1, 3, 4]].tobytes() == keep[k][[1, 3, 4]].tobytes() and (got[[0, 2]] != keep[k][[0, 2]]).any() and np.isfinite(got).all()
    a.close(), b.close()


def test_six_blocks_equal_the_block_alone_and_sensors_alone_equal_the_sensor_entry():
    import sim_dyn_cases as D
    from gymnasium_robotics_amd.core import stream_ptr

    alone = scene("arm", body_dynamics=ALL)
    full = scene("arm", body_dynamics=ALL, outputs=S.ALL_OUTPUTS + D.DYNAMICS, jac_sites=("ee",), contacts=("contact_geom", "contact_force"), applied=("xipos",), sensors="all")
    alone.step(3), full.step(3)
    assert all(host(getattr(full, k)).tobytes() == host(getattr(alone, k)).tobytes() for k in ALL)
    sns = scene("arm", sensors="all")      # the fifth block alone, through its own entry and through the new one with a null sixth block
    sns.forward()
    want = host(sns.sensor_data)
    sns.sensor_data.fill_(float("nan"))
    sns.qacc_warmstart.zero_()      # (the first launch has updated it: the same start for the second)
    bufs = sns._make_bufs(None)
    assert sns._L.grx_sim_step_wrn(sns._h, None, ctypes.byref(bufs), None, None, None, ctypes.byref(sns._sns), None, N, 0, 1, stream_ptr(sns.device)) == 0
    assert host(sns.sensor_data).tobytes() == want.tobytes()
    alone.close(), full.close(), sns.close()


def test_c_abi_checks_force_rows_on_the_host():
    from gymnasium_robotics_amd import _native
    from gymnasium_robotics_amd import sim as simmod
    from gymnasium_robotics_amd.core import stream_ptr

    sim = scene("arm", sensors="all")
    sim.forward()
    keep, bufs, T, O = host(sim.sensor_data), sim._make_bufs(None), simmod.SENSOR_TYPES.index, simmod.SENSOR_OBJECTS.index
    cut = np.zeros(1, np.float32)

    def call(entry, spec):
        spec = np.ascontiguousarray(spec, dtype=np.int32).reshape(-1, 4)
        blk = _native.SimSensorsStruct(spec=spec.ctypes.data, cutoff=cut.ctypes.data, nsensor=1, ndata=3, data=sim.sensor_data.data_ptr())
        tail = (None,) if entry == "grx_sim_step_wrn" else ()
        rc = getattr(sim._L, entry)(sim._h, None, ctypes.byref(bufs), None, None, None, ctypes.byref(blk), *tail, N, 0, 1, stream_ptr(sim.device))
        return rc, sim._L.grx_last_error().decode()

    for entry, spec, why in (("grx_sim_step_wrn", [T("force"), O("xbody"), 1, 0], "does not read an object"), ("grx_sim_step_wrn", [T("torque"), O("site"), sim.nsite, 0], "is outside"),
                             ("grx_sim_step_sns", [T("force"), O("site"), 0, 0], "grx_sim_step_wrn is the call")):
        rc, msg = call(entry, spec)
        assert rc == -1 and msg.startswith("grx_sim_step_sns:") and why in msg, (why, msg)
    assert host(sim.sensor_data).tobytes() == keep.tobytes()      # nothing was launched
    sim.close()
