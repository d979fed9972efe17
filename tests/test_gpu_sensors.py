"""The sensor block of grx.BatchedSim on the GPU (pytest -m gpu): sensor_data against the fp64 reference (tests/sensor_refs.py) on the tree cases of tests/sensor_cases.py, the
pass rule after step(), and the readings of the scenes with a floor and actuators against closed forms.  N = 5 worlds per case, 13 once.  The preconditions (the reference's
jitter and its own error below a tenth of every bound, for every world compared here) are asserted in tests/test_cpu_sensors.py.  Every row starts as NaN: the launch owes
every element.

Bounds: positions, quaternions (up to sign) and axes engine_matrix_cases.BOUND absolute; velocity types BOUND (1 + |qvel|_1); joint and actuator types BOUND max(1, |value|);
acceleration types twice the larger worst figure of tests/golden/sensor_errors.json (emulator, MI355X) times (1 + |g| + |want|_inf), which may not exceed 1e-3.  Every figure
is printed before it is asserted."""
import numpy as np
import pytest

import engine_matrix_cases as C
import sensor_cases as SC
import sensor_refs as SR
import sim_cases as S
from test_cpu_sensors import acc_bound

pytestmark = pytest.mark.gpu

N = SC.N_WORLDS
G_ARM = 9.81      # the arm scene's gravity (MuJoCo's default)


def tree_sim(name, n, **kw):
    import torch

    import gymnasium_robotics_amd as grx

    assert torch.cuda.is_available(), "these tests need the GPU"
    case = SC.CASES[name]
    sim = grx.BatchedSim(case.model, n, sensors=tuple(s["name"] for s in case.sensors), **kw)
    st = case.states(n)
    sim.qpos.copy_(torch.from_numpy(st["qpos"].astype(np.float32)))
    sim.qvel.copy_(torch.from_numpy(st["qvel"].astype(np.float32)))
    sim.sensor_data.fill_(float("nan"))
    return sim


def scene_sim(scene, n=N, sensors="all", st=None, **kw):
    import torch

    import gymnasium_robotics_amd as grx

    assert torch.cuda.is_available(), "these tests need the GPU"
    sc = SC.SCENES[scene]
    sim = grx.BatchedSim(sc.model, n, sensors=sensors, **kw)
    st = sc.states(n) if st is None else st
    for k in ("qpos", "qvel", "ctrl", "mocap_pos", "mocap_quat"):
        getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)).reshape(getattr(sim, k).shape))
    sim.qacc_warmstart.zero_()
    sim.sensor_data.fill_(float("nan"))
    return sim


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


_ROWS = {}


def forward_rows(name, n):
    if (name, n) not in _ROWS:
        sim = tree_sim(name, n)
        sim.forward()
        _ROWS[(name, n)] = host(sim.sensor_data)
        sim.close()
    return _ROWS[(name, n)]


@pytest.mark.parametrize("name,n", SC.RUNS)
def test_forward_matches_reference(name, n):
    case, rows, ref, st = SC.CASES[name], forward_rows(name, n), SC.reference(name, n), SC.CASES[name].states(n)
    assert np.isfinite(rows).all()
    adr, _ = SR.layout(case.sensors)
    worst = {}
    for i in range(n):
        r = SC.compare(case, rows[i], ref["data"][i], st["qvel"][i], acc_bound())
        for s in case.sensors:
            a, d = adr[s["name"]]
            worst[s["type"]] = max(worst.get(s["type"], 0.0), float(r[a:a + d].max()))
    fig = max(float(SC.compare(case, rows[i], ref["data"][i], st["qvel"][i], 1.0)[SC.acc_mask(case)].max()) for i in range(n))
    print(name, n, "error / bound per type", {k: f"{v:.3g}" for k, v in worst.items()}, "acceleration figure", fig, "bound", acc_bound())
    assert acc_bound() <= SC.ACC_MAX
    assert max(worst.values()) <= 1.0, worst


def test_thirteen_worlds_equal_the_first_five_bit_for_bit():
    assert forward_rows(SC.RUN13, 13)[:N].tobytes() == forward_rows(SC.RUN13, N).tobytes()


@pytest.mark.parametrize("scene,nstep", [("arm", 1), ("arm", 4), ("rk4", 1), ("rk4", 4)])
def test_step_reads_the_sensor_pass_of_the_last_substep(scene, nstep):
    """sensor_data after step(n) is sensor_data after step(n - 1) and forward() from the same start: bit for bit on the Euler scene, within the velocity bound under RK4 (its
    first stage evaluates at the substep's start state, which forward() sees after a store and a load of the warm start)"""
    a = scene_sim(scene)
    a.step(nstep)
    got = host(a.sensor_data)
    b = scene_sim(scene)
    if nstep > 1:
        b.step(nstep - 1)
    b.sensor_data.fill_(float("nan"))
    qvel = host(b.qvel)
    b.forward()
    want = host(b.sensor_data)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    if scene == "arm":
        assert got.tobytes() == want.tobytes()
    else:
        bound = C.BOUND * (1.0 + np.abs(qvel).sum(axis=1, keepdims=True))
        print(scene, nstep, "worst / bound", float((np.abs(got - want) / bound).max()))
        assert (np.abs(got - want) <= bound).all()
    a.close(), b.close()


def test_rk4_readings_are_the_first_stage_not_the_fourth():
    """after step(1) framepos of a moving site is its position at the substep's START, site_xpos of the same launch the fourth stage's trial position"""
    sim = scene_sim("rk4", outputs=("site_xpos",))
    start = scene_sim("rk4")
    start.forward()
    sim.step(1)
    adr, dim = sim.sensor_adr("tip_pos")
    pos, xpos, pos0 = host(sim.sensor_data)[:, adr:adr + dim], host(sim.site_xpos)[:, sim.site_id("tip")], host(start.sensor_data)[:, adr:adr + dim]
    print("framepos vs site_xpos", np.abs(pos - xpos).max(axis=1), "framepos vs the start", np.abs(pos - pos0).max())
    assert (np.abs(pos - xpos).max(axis=1) > C.BOUND).all()
    assert np.abs(pos - pos0).max() <= C.BOUND
    sim.close(), start.close()


def _resting(st, n):
    st = {k: v.copy() for k, v in st.items()}
    st["qvel"][:, 4:10] = 0.0      # the box starts at rest, pressed into the floor; it settles within a few time constants of the contact
    return st


def test_resting_box_reads_gravity_in_its_own_frame():
    sc = SC.SCENES["arm"]
    sim = scene_sim("arm", st=_resting(sc.states(N), N), outputs=("site_xmat",))
    sim.step(500)
    a, d = sim.sensor_adr("box_acc")
    got, Rm = host(sim.sensor_data)[:, a:a + d], host(sim.site_xmat)[:, sim.site_id("pad")].reshape(N, 3, 3)
    want = G_ARM * Rm[:, 2, :]      # R'(0, 0, |g|)
    fig = np.abs(got - want).max(axis=1) / (1.0 + G_ARM + np.abs(want).max(axis=1))
    print("resting accelerometer", got, "figure", fig, "bound", acc_bound())
    assert (fig <= acc_bound()).all()
    a, d = sim.sensor_adr("box_linacc")      # the same in world coordinates, on the xbody
    lin = host(sim.sensor_data)[:, a:a + d]
    assert (np.abs(lin - [0.0, 0.0, G_ARM]).max(axis=1) / (1.0 + 2.0 * G_ARM) <= acc_bound()).all()
    sim.close()


def test_actuator_force_at_the_clamp_is_the_forcerange_limit():
    sc = SC.SCENES["arm"]
    st = {k: v.copy() for k, v in sc.states(N).items()}
    st["qpos"][0, 0], st["ctrl"][0, 0] = -1.5, 1.2      # kp (clamp(ctrl) - q) = 20 x 2.5: far above the range
    st["qpos"][1, 0], st["ctrl"][1, 0] = 1.5, -1.2
    st["qpos"][2, 0], st["ctrl"][2, 0] = 0.25, 0.3125   # 20 x 0.0625 = 1.25: inside it, exact in fp32
    st["qvel"][:3, 0] = 0.0
    sim = scene_sim("arm", st=st)
    sim.forward()
    data = host(sim.sensor_data)
    frc, afrc = (data[:, sim.sensor_adr(k)[0]] for k in ("a1_frc", "j1_afrc"))
    assert frc[0] == SC.ARM_FORCERANGE and frc[1] == -SC.ARM_FORCERANGE and frc[2] == 1.25
    assert (afrc[:3] == frc[:3]).all()      # gear 1: the joint sees the same force
    pos, vel = (data[:, sim.sensor_adr(k)[0]] for k in ("a1_pos", "a1_vel"))
    assert (pos == st["qpos"][:, 0].astype(np.float32)).all() and (vel == st["qvel"][:, 0].astype(np.float32)).all()
    sim.close()


def test_masked_out_worlds_keep_their_rows_bit_for_bit():
    import torch

    sim = scene_sim("arm")
    pattern = torch.arange(sim.sensor_data.numel(), dtype=torch.float32, device=sim.device).reshape(sim.sensor_data.shape) * 0.5 - 7.0
    sim.sensor_data.copy_(pattern)
    mask = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8, device=sim.device)
    sim.step(2, mask=mask)
    got, keep = host(sim.sensor_data), host(pattern)
    assert got[[1, 3, 4]].tobytes() == keep[[1, 3, 4]].tobytes()
    assert (got[[0, 2]] != keep[[0, 2]]).all()
    full = scene_sim("arm")
    full.step(2)
    assert got[[0, 2]].tobytes() == host(full.sensor_data)[[0, 2]].tobytes()
    sim.close(), full.close()


def test_resting_accelerometer_follows_the_worlds_own_gravity():
    import torch

    sc = SC.SCENES["arm"]
    sim = scene_sim("arm", st=_resting(sc.states(N), N), model_params=("gravity",))
    gz = np.array([-9.81 * f for f in (0.8, 0.9, 1.0, 1.1, 1.2)], dtype=np.float32)
    sim.params.gravity[:, 2] = torch.from_numpy(gz).to(sim.device)
    sim.commit_params()
    sim.step(500)
    assert not host(sim.params_invalid).any()
    a, d = sim.sensor_adr("box_linacc")
    got = host(sim.sensor_data)[:, a:a + d]
    fig = np.abs(got - np.stack([np.zeros(N), np.zeros(N), -gz], axis=1)).max(axis=1) / (1.0 + 2.0 * np.abs(gz))
    print("per-world gravity", got[:, 2], "figure", fig)
    assert (fig <= acc_bound()).all()
    sim.close()


def test_applied_force_on_a_falling_body_reads_f_over_m():
    import torch

    case = SC.CASES["free-alone"]
    sim = tree_sim("free-alone", N, applied=("xfrc_applied",), outputs=("site_xmat",))
    sim.qvel.zero_()      # no rotation: a force through the centre of mass leaves R'(g + f / m - g)
    b = sim.body_id("fr")
    f = np.array([[1.5, -2.0, 4.0], [0.0, 0.0, 12.0], [-3.0, 0.5, 0.0], [0.25, 0.25, -6.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    sim.xfrc_applied[:, b, :3] = torch.from_numpy(f).to(sim.device)
    sim.forward()
    mass = float(sum(x["mass"] for x in case.tree["bodies"]))      # the root and its joint-less child
    a, d = sim.sensor_adr("hub_accelerometer")
    got, Rm = host(sim.sensor_data)[:, a:a + d], host(sim.site_xmat)[:, sim.site_id("hub")].reshape(N, 3, 3)
    want = np.einsum("nji,nj->ni", Rm.astype(np.float64), f.astype(np.float64) / mass)
    g = float(np.linalg.norm(case.tree["gravity"]))
    fig = np.abs(got - want).max(axis=1) / (1.0 + g + np.abs(want).max(axis=1))
    print("R'f / m", want, "figure", fig)
    assert (fig <= acc_bound()).all()
    sim.close()


def test_overflow_rerun_writes_the_row():
    sim = scene_sim("pile", outputs=("ncon",))
    sim.step(2)
    data, ncon = host(sim.sensor_data), host(sim.ncon)
    print("ncon", ncon)
    assert (ncon[1:] > S.PILE_MAXCON).all() and ncon[0] <= S.PILE_MAXCON      # worlds 1 .. 4 ran again on the large tables
    assert np.isfinite(data).all()
    a, d = sim.sensor_adr("acc0")
    assert (np.abs(data[:, a:a + d]) < 1e3).all()
    sim.close()


def test_five_blocks_equal_sensors_alone_on_the_sensor_row():
    import sim_dyn_cases as D

    alone = scene_sim("arm")
    alone.step(3)
    full = scene_sim("arm", outputs=S.ALL_OUTPUTS + D.DYNAMICS, jac_sites=("ee",), contacts=("contact_geom", "contact_force"), applied=("xipos",))
    full.step(3)
    assert host(full.sensor_data).tobytes() == host(alone.sensor_data).tobytes()
    assert np.isfinite(host(full.xipos)).all() and np.isfinite(host(full.qfrc_bias)).all()
    alone.close(), full.close()


def test_c_abi_checks_the_host_table():
    """the table is checked on the host, before anything is uploaded or launched; a block without data launches what grx_sim_step_frc launches"""
    import ctypes

    import torch

    from gymnasium_robotics_amd import _native
    from gymnasium_robotics_amd import sim as simmod
    from gymnasium_robotics_amd.core import stream_ptr

    sim = scene_sim("arm")
    sim.forward()
    torch.cuda.synchronize()
    L, T, O = sim._L, simmod.SENSOR_TYPES.index, simmod.SENSOR_OBJECTS.index
    keep = host(sim.sensor_data)
    bufs = sim._make_bufs(None)      # the rows alone, no overflow lane: what a C caller passes

    def call(spec, cutoff=None, ndata=None, data=True):
        spec = np.ascontiguousarray(spec, dtype=np.int32).reshape(-1, 4)
        cut = np.zeros(len(spec), np.float32) if cutoff is None else np.ascontiguousarray(cutoff, dtype=np.float32)
        nd = int(sum(4 if t == 7 else (3 if t >= 6 else 1) for t in spec[:, 0])) if ndata is None else ndata
        blk = _native.SimSensorsStruct(spec=spec.ctypes.data, cutoff=cut.ctypes.data, nsensor=len(spec), ndata=nd, data=sim.sensor_data.data_ptr() if data else None)
        rc = L.grx_sim_step_sns(sim._h, None, ctypes.byref(bufs), None, None, None, ctypes.byref(blk), sim.num_worlds, 0, 1, stream_ptr(sim.device))
        torch.cuda.synchronize()
        return rc, L.grx_last_error().decode()

    ee, j1 = sim.site_id("ee"), sim.model.names["joint"]["j1"]
    bad = {"unknown type": [[99, O("site"), ee, 0]], "unknown object type": [[T("framepos"), 9, ee, 0]], "does not read an object": [[T("accelerometer"), O("xbody"), 1, 0]],
           "is outside": [[T("framepos"), O("site"), sim.nsite, 0]], "free or ball joint": [[T("jointpos"), O("joint"), sim.model.names["joint"]["boxj"], 0]],
           "the rows before it end at": [[T("jointpos"), O("joint"), j1, 0], [T("framepos"), O("site"), ee, 2]]}
    for why, spec in bad.items():
        rc, msg = call(spec)
        assert rc == -1 and msg.startswith("grx_sim_step_sns: sensor") and why in msg, (why, msg)
    rc, msg = call([[T("jointpos"), O("joint"), j1, 0]], ndata=3)
    assert rc == -1 and "ndata = 3" in msg, msg
    rc, msg = call([[T("jointpos"), O("joint"), j1, 0]], cutoff=[-1.0])
    assert rc == -1 and "cutoff" in msg, msg
    assert host(sim.sensor_data).tobytes() == keep.tobytes()      # nothing was launched
    assert call([[T("jointpos"), O("joint"), j1, 0]], data=False)[0] == 0      # no data: the launch of the call without the block
    assert host(sim.sensor_data).tobytes() == keep.tobytes()
    sim.close()
