"""Cameras on the device (BatchedSim.render / render_pose, grx_sim_render) against the fp64 reference and under the acceptance rule of tests/ray_cases.py, on the pixel rays
of tests/camera_cases.py.  The images are filled with NaN / a sentinel before every launch: a pixel the launch does not write fails the finiteness check."""
import ctypes

import numpy as np
import pytest

import camera_cases as K
import engine_matrix_cases as C
import ray_cases as R
from test_gpu_rays import SENTINEL, _sim

pytestmark = pytest.mark.gpu
FOVY = 60.0


def _images(call, sim, n_cams, h, w, *args, **kw):
    """call(*args, h, w, segmentation=True, out=NaN / sentinel-filled images); host arrays back"""
    import torch

    out = (torch.full((sim.num_worlds, n_cams, h, w), float("nan"), device=sim.device), torch.full((sim.num_worlds, n_cams, h, w), SENTINEL, dtype=torch.int32, device=sim.device))
    depth, seg = call(*args, h, w, segmentation=True, out=out, **kw)
    torch.cuda.synchronize()
    return depth.cpu().numpy(), seg.cpu().numpy()


def _accept(tag, model, gx, gm, pose, fovy, images, seed, **kw):
    """one image (depth, seg) [H, W] against the reference's cast of its pixel fan; returns the reference geoms of the compared pixels"""
    o, d = K.fan(*pose, fovy, *images[0].shape)
    want_depth, want_seg = R.cast(model, gx, gm, o, d, **kw)
    compared = R.compared_mask(model, gx, gm, o, d, want_depth, want_seg, seed, **kw)
    R.accept(tag, model, images[0].ravel(), images[1].ravel(), want_depth, want_seg, compared, {})
    assert compared.mean() >= R.MIN_SHARE, (tag, compared.mean())
    return want_seg[compared]


@pytest.fixture(scope="module")
def crowd():
    """crowd-mixed's five worlds after forward(), their reference worlds, and the poses [5, 2, 3 / 9] of camera A (above the crowd) and B (inside it), fp32 values in fp64"""
    var = R.M.group(R.SCENE).variants[0]
    sim = _sim(var.model, len(var.idx), var.q0, var.v0)
    sim.forward()
    worlds = [R.world(0, i) for i in range(len(var.idx))]
    pos, mat = np.zeros((len(worlds), 2, 3)), np.zeros((len(worlds), 2, 9))
    for i, w in enumerate(worlds):
        c = w.gxpos[R.geoms_of(w.model).type != 0].mean(axis=0)
        pos[i] = c + [0.3, -0.4, 2.0], c + [0.05, 0.02, 0.1]
        mat[i] = K.look_at(pos[i, 0], c), K.look_at(pos[i, 1], c + [0.3, 0.2, -0.3])
    yield sim, worlds, C.f32(pos), C.f32(mat)
    sim.close()


@pytest.mark.parametrize("h, w", [(1, 1), (8, 8), (9, 13), (24, 40)])
def test_render_pose_against_the_reference(crowd, h, w):
    """one pixel, one 8 x 8 tile (half a 16 x 4 one), ragged edge tiles in both shapes, and several tiles per wave; camera B, inside a bounding sphere, at the two larger sizes"""
    sim, worlds, pos, mat = crowd
    depth, seg = _images(sim.render_pose, sim, 2, h, w, pos, mat, FOVY)
    seen = set()
    for i, wd in enumerate(worlds):
        for j in (0, 1) if h >= 9 else (0,):
            seen |= set(_accept(("mi355x", "AB"[j], h, w, i), wd.model, wd.gxpos, wd.gxmat, (pos[i, j], mat[i, j]), FOVY, (depth[i, j], seg[i, j]), (wd.index, 10 + j, h)).tolist())
    assert (h, w) != (24, 40) or len(seen - {-1}) >= 13


@pytest.mark.parametrize("h, w", [(24, 40), (9, 13)])
def test_binning_changes_no_bit(crowd, h, w):
    """a conservative bin drops no geom a pixel can see: the binned image is the unbinned one bit for bit, in both tile shapes"""
    sim, _, pos, mat = crowd
    want = _images(sim.render_pose, sim, 2, h, w, pos, mat, FOVY, binning=False)
    assert (want[1] >= 0).any() and (want[1] == -1).any()
    for tile in ("16x4", "8x8"):
        got = _images(sim.render_pose, sim, 2, h, w, pos, mat, FOVY, tile=tile)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), tile


@pytest.fixture(scope="module")
def rig():
    """tests/camera_cases.py XML in five worlds at different hinge angles, and the oracle of the same model"""
    from oracle.oracle_sim import OracleSim

    model = C.compile_xml(K.XML)
    angles = C.f32(np.array([[0.0], [0.7], [-1.1], [1.2], [3.0]]))
    sim = _sim(model, 5, angles, np.full((5, 1), 1.5))
    yield sim, model, OracleSim(model), angles
    sim.close()


@pytest.mark.parametrize("nstep", [0, 2])
def test_named_cameras_follow_their_bodies(rig, nstep):
    """the fused camera on the hinged arm and the default-class one in the world, and render_pose fed the pose numpy composes from xpos / xquat and info["camera"], see what
    the reference sees from the oracle's pose: after forward() the current one, after step(2) that of the last substep's position stage (MjData's), one substep stale"""
    import torch

    sim, model, orc, angles = rig
    sim.qpos.copy_(torch.from_numpy(angles.astype(np.float32)))
    sim.qvel.fill_(1.5)
    sim.qacc_warmstart.zero_()
    sim.step(nstep) if nstep else sim.forward()
    names, arm = ["eye", "overview"], sim.body_id("arm")      # the eye sits inside its own body's `head`: it looks past the arm's geoms
    rows = [model.info["camera"][sim.camera_id(n)] for n in names]
    named = _images(sim.render, sim, 2, 12, 20, names, exclude_body=[arm, -1])
    xpos, xquat = sim.xpos.cpu().numpy().astype(np.float64), sim.xquat.cpu().numpy().astype(np.float64)
    pos, mat = (np.stack([[K.pose(r, xpos[i], xquat[i])[k] for r in rows] for i in range(5)]) for k in (0, 1))
    posed = _images(sim.render_pose, sim, 2, 12, 20, pos, mat, [r["fovy"] for r in rows], exclude_body=[arm, -1])
    for i in range(5):
        orc.reset_data()
        orc.qpos[:], orc.qvel[:] = angles[i], 1.5
        orc.step(nstep) if nstep else orc.forward()
        gx, gm = orc.geom_xpos.reshape(-1, 3).copy(), orc.geom_xmat.reshape(-1, 9).copy()
        for j, r in enumerate(rows):
            for got in (named, posed):      # both under the rule, against the reference's view from the oracle's pose
                _accept(("mi355x", names[j], nstep, i), model, gx, gm, K.pose(r, orc.xpos, orc.xquat), r["fovy"], (got[0][i, j], got[1][i, j]), (i, j, nstep), **(dict(exclude_body=arm) if j == 0 else {}))


def test_filters_and_masked_rows(rig):
    """the eye sits inside its own body's `head`, which fills its image until exclude_own_body removes it; max_dist is a bound on depth; a masked world keeps its bits"""
    import torch

    sim, model, orc, angles = rig
    sim.qpos.copy_(torch.from_numpy(angles.astype(np.float32)))
    sim.forward()
    head, link = sim.geom_id("head"), sim.geom_id("link")
    depth, seg = _images(sim.render, sim, 1, 16, 16, "eye")
    own = _images(sim.render, sim, 1, 16, 16, "eye", exclude_own_body=True)
    assert (seg == head).all() and not np.isin(own[1], (head, link)).any() and (own[1] >= 0).any()
    cut = float(np.median(own[0][own[0] > 0]))
    near = _images(sim.render, sim, 1, 16, 16, "eye", exclude_own_body=True, max_dist=cut)
    assert np.array_equal(near[1], np.where(own[0] > cut, -1, own[1])) and np.array_equal(near[0], np.where(own[0] > cut, -1.0, own[0])) and (near[1] >= 0).any()
    mask = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8, device=sim.device)
    kept = _images(sim.render, sim, 1, 16, 16, "eye", mask=mask)
    assert np.isnan(kept[0][[1, 3, 4]]).all() and (kept[1][[1, 3, 4]] == SENTINEL).all() and np.array_equal(kept[0][[0, 2]], depth[[0, 2]])
    fresh = sim.render("eye", 16, 16, mask=mask).cpu().numpy()      # without out=: the images of the worlds the mask leaves out read "no hit"
    assert (fresh[[1, 3, 4]] == -1.0).all() and np.array_equal(fresh[[0, 2]], depth[[0, 2]])


def test_one_geom_more_than_a_staging_pass():
    """128 spheres in a grid fill one staging pass; the 129th, alone in a second pass, hangs above them: it must be seen, and the second pass must keep what the first saw"""
    from oracle.oracle_sim import OracleSim

    n = 129      # GRX_CAM_STAGE + 1
    balls = "".join(f'<geom type="sphere" size="{0.05 if k < n - 1 else 0.12}" pos="{0.15 * (k % 12)} {0.15 * (k // 12)} {0.05 if k < n - 1 else 0.5}"/>' for k in range(n))
    model = C.compile_xml(f'<mujoco><worldbody>{balls}<body pos="-1 -1 1"><freejoint/><geom type="sphere" size="0.05" mass="1"/></body></worldbody></mujoco>')
    orc = OracleSim(model)
    orc.forward()
    gx, gm = orc.geom_xpos.reshape(-1, 3).copy(), orc.geom_xmat.reshape(-1, 9).copy()
    sim = _sim(model, 5, np.tile(orc.qpos, (5, 1)), np.zeros((5, orc.nv)))
    try:
        sim.forward()
        pos = C.f32(gx[n - 1] + [0.2, 0.1, 2.0])
        mat = C.f32(K.look_at(pos, gx[n - 1]))
        depth, seg = _images(sim.render_pose, sim, 1, 16, 16, pos[None], mat[None], 50.0)
        for i in range(5):
            seen = _accept(("mi355x", "passes", i), model, gx, gm, (pos, mat), 50.0, (depth[i, 0], seg[i, 0]), (n,))
        assert len(gx) == n + 1 and (seen == n - 1).any() and len(set(seen.tolist()) - {-1, n - 1}) >= 5
    finally:
        sim.close()


def test_c_abi_error_returns(rig):
    import torch

    from gymnasium_robotics_amd import _native

    sim, model, orc, angles = rig
    sim.forward()
    L = sim._L
    depth = torch.zeros((5, 2, 4, 4), device=sim.device)
    body, cpos, cquat, fovy = (ctypes.c_int * 2)(0, 1), (ctypes.c_float * 6)(0, 0, 2, 0, 0, 0.5), (ctypes.c_float * 8)(1, 0, 0, 0, 1, 0, 0, 0), (ctypes.c_float * 2)(45, 45)
    ptr = lambda x: ctypes.cast(x, ctypes.c_void_p).value
    full = dict(xpos=sim.xpos.data_ptr(), xquat=sim.xquat.data_ptr(), cam_body=ptr(body), cam_pos=ptr(cpos), cam_quat=ptr(cquat), cam_fovy=ptr(fovy), depth=depth.data_ptr(), include_static=1)

    def refused(word, m=sim._h, n=5, k=2, hh=4, ww=4, block=True, **kw):
        b = _native.SimCamerasStruct(**{**full, **kw})
        assert L.grx_sim_render(m, ctypes.byref(b) if block else None, n, k, hh, ww, None) == -1
        assert word in L.grx_last_error().decode(), L.grx_last_error()

    for word, kw in (("null model", dict(m=None)), ("null camera block", dict(block=False)), ("null body poses", dict(xquat=None)), ("null depth", dict(depth=None)),
                     ("null camera poses", dict(cam_quat=None)), ("pose_pos without pose_mat", dict(pose_pos=depth.data_ptr())), ("null cam_fovy", dict(cam_fovy=None)),
                     ("n_worlds < 1", dict(n=0)), ("outside 1 .. 16", dict(k=0)), ("outside 1 .. 16", dict(k=17)), ("outside 1 .. 1024", dict(hh=0)), ("outside 1 .. 1024", dict(ww=1025))):
        refused(word, **kw)
    for table, at, bad, good, word in ((fovy, 1, 180.0, 45.0, "outside (0, 180)"), (body, 1, sim.nbody, 1, "outside [0, nbody)"), (cquat, 4, 0.0, 1.0, "zero or not finite")):
        table[at] = bad
        refused(word)
        table[at] = good
    assert L.grx_sim_render(sim._h, ctypes.byref(_native.SimCamerasStruct(**full)), 5, 2, 4, 4, None) == 0      # seg is optional
    torch.cuda.synchronize()
    assert (depth.cpu().numpy() != 0).all()
