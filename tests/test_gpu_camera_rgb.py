"""Colour and surface-normal images on the device (render(rgb=True, normals=True), grx_sim_render_rgb) against tests/shade_refs.py, on the scenes of tests/test_gpu_camera.py; images start as NaN / a sentinel."""
import contextlib
import ctypes

import numpy as np
import pytest

import camera_cases as K
import engine_matrix_cases as C
import ray_cases as R
import shade_refs as S
from gymnasium_robotics_amd import _native
from test_gpu_camera import FOVY, crowd  # noqa: F401  (the fixture)
from test_gpu_rays import SENTINEL, _sim

pytestmark = pytest.mark.gpu
LIGHT = dict(ambient=0.25, diffuse=0.6, sun=(0.3, -0.5, -0.8), sun_diffuse=0.4, background=(0.1, 0.6, 0.9))
FLAT = dict(ambient=1.0, diffuse=0.0)      # s = 1: whatever the normal, a pixel is its geom's colour, rounded; _flat: the RGBA levels [seg.size, 4] of the image seg then
_flat = lambda seg, colors, background: S.shade(np.zeros((seg.size, 3)), np.ones((seg.size, 3)), seg.ravel(), colors, background=background, **FLAT)
BYTE, NORMAL_BOUND = 0x5A, 2e-5      # the rgb image before a launch; |n_device - n_reference|_inf: 4 x the worst measured on the MI355X (tests/golden/camera_rgb_errors.json), rounded up to one digit


def _images(call, sim, n_cams, h, w, *args, **kw):
    """call(*args, h, w, segmentation, rgb, normals, out=filled images), arrays in kw as device tensors; host arrays (depth, seg, rgb, normal) back"""
    import torch
    full = lambda tail, value, dtype=torch.float32: torch.full((sim.num_worlds, n_cams, h, w) + tail, value, dtype=dtype, device=sim.device)
    kw = {k: torch.tensor(v, dtype=torch.float32, device=sim.device) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    got = call(*args, h, w, segmentation=True, rgb=True, normals=True, out=(full((), np.nan), full((), SENTINEL, torch.int32), full((4,), BYTE, torch.uint8), full((3,), np.nan)), **kw)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in got]


@pytest.mark.parametrize("h, w", [(1, 1), (9, 13), (24, 40)])
def test_normals_colours_and_modes_against_the_reference(crowd, h, w):
    """per-world colours (some outside [0, 1]: clamped) and a sun.  Compared: the pixels ray_cases.compared_mask keeps, minus the crease pixels -- those where the
    reference's own normal changes by more than 1e-3 when the ray is shifted by 1e-3 pixel in u or v.  Camera B, inside a bounding sphere, is left out at 1 x 1 as in
    test_gpu_camera (one uncompared pixel is a share of 0).  Camera C, 0.8 m above the crowd, is added at 24 x 40: from A's 2 m, 1e-3 pixel (1e-4 m) turns the normal of a
    5 cm sphere by 2e-3, so every pixel of a sphere, capsule or ellipsoid is a crease pixel; from C all seven geom types are compared"""
    sim, worlds, pos, mat = crowd
    centre = [wd.gxpos[R.geoms_of(wd.model).type != 0].mean(axis=0) for wd in worlds]
    pos = np.concatenate([pos, C.f32(np.array([c + [0.05, -0.1, 0.8] for c in centre]))[:, None]], axis=1)
    mat = np.concatenate([mat, C.f32(np.array([K.look_at(p, c) for p, c in zip(pos[:, 2], centre)]))[:, None]], axis=1)
    kw = dict(colors=C.f32(np.random.default_rng(5).uniform(-0.1, 1.2, (len(worlds), R.geoms_of(worlds[0].model).n, 3))), **LIGHT)
    depth, seg, rgb, nrm = _images(sim.render_pose, sim, 3, h, w, pos, mat, FOVY, **kw)
    base = [x.cpu().numpy() for x in sim.render_pose(pos, mat, FOVY, h, w, segmentation=True)] + [rgb, nrm]      # depth and seg are the depth kernel's bits, and every image keeps its bits without binning and with 16 x 4 tiles
    for mode in (dict(), dict(binning=False), dict(tile="16x4")):
        assert all(np.array_equal(x, y) for x, y in zip(_images(sim.render_pose, sim, 3, h, w, pos, mat, FOVY, **kw, **mode), base)), mode
    seen, step = set(), 2e-3 * np.tan(np.radians(FOVY) / 2.0) / h      # step: what 1e-3 pixel adds to the camera-frame x or y of a direction
    for i, wd in enumerate(worlds):
        G, cast = R.geoms_of(wd.model), lambda o, d: R.cast(wd.model, wd.gxpos, wd.gxmat, o, d)
        for j in range(3 if h >= 24 else 2 if h >= 9 else 1):
            tag, (o, d) = ("mi355x", "ABC"[j], h, w, i), K.fan(pos[i, j], mat[i, j], FOVY, h, w)
            want_depth, want_seg = cast(o, d)
            want_n = S.normals(wd.model, wd.gxpos, wd.gxmat, o, d, want_depth, want_seg)
            keep = R.compared_mask(wd.model, wd.gxpos, wd.gxmat, o, d, want_depth, want_seg, (wd.index, 10 + j, h))
            for shifted in [d + sign * step * axis for axis in mat[i, j].reshape(3, 3).T[:2] for sign in (1, -1)]:
                keep &= np.abs(S.normals(wd.model, wd.gxpos, wd.gxmat, o, shifted, *cast(o, shifted)) - want_n).max(axis=1) <= 1e-3
            assert keep.mean() >= R.MIN_SHARE, (tag, keep.mean())
            R.accept(tag, wd.model, depth[i, j].ravel(), seg[i, j].ravel(), want_depth, want_seg, keep, {})
            err, off = np.abs(nrm[i, j].reshape(-1, 3) - want_n).max(axis=1), np.abs(rgb[i, j].reshape(-1, 4) - S.shade(want_n, d, want_seg, kw["colors"][i], **LIGHT)).max(axis=1)
            kind = np.where(keep & (want_seg >= 0), G.type[want_seg], -1)
            print(f"{tag}: kept {int(keep.sum())} / {len(keep)}, worst colour difference {off[keep].max()} level(s), worst normal error", {R.TYPE_NAMES[t]: float("%.3g" % err[kind == t].max()) for t in sorted(set(kind.tolist()) - {-1})})
            assert (err[keep] <= NORMAL_BOUND).all() and (off[keep] <= 1).all(), (tag, err[keep].max(), off[keep].max())      # (off covers alpha: 255 against 0)
            seen |= set(kind.tolist()) - {-1}
    assert NORMAL_BOUND * 255.0 < 0.1 and ((h, w) != (24, 40) or seen == set(G.type.tolist()))      # within the bound c s moves by far less than a level: one level is the rounding's; every geom type was compared


def test_the_129th_geom_is_shaded_in_its_own_pass():
    """test_gpu_camera's 128 + 1 spheres, each its own colour, flat light: a pixel is the colour of the geom seg names, whichever pass staged it; a miss the background, alpha 0, normal 0"""
    from oracle.oracle_sim import OracleSim
    n = 129      # GRX_CAM_STAGE + 1
    balls = "".join(f'<geom type="sphere" size="{0.05 if k < n - 1 else 0.12}" pos="{0.15 * (k % 12)} {0.15 * (k // 12)} {0.05 if k < n - 1 else 0.5}"/>' for k in range(n))
    model = C.compile_xml(f'<mujoco><worldbody>{balls}<body pos="-1 -1 1"><freejoint/><geom type="sphere" size="0.05" mass="1"/></body></worldbody></mujoco>')
    orc = OracleSim(model)
    orc.forward()
    top, colors = orc.geom_xpos.reshape(-1, 3)[n - 1].copy(), np.array([[(7 * k) % 256, (13 * k) % 256, (29 * k + 1) % 256] for k in range(n + 1)]) / 255.0
    with contextlib.closing(_sim(model, 5, np.tile(orc.qpos, (5, 1)), np.zeros((5, orc.nv)))) as sim:
        sim.forward()
        pos = C.f32(top + [0.2, 0.1, 2.0])
        depth, seg, rgb, nrm = _images(sim.render_pose, sim, 1, 16, 16, pos[None], C.f32(K.look_at(pos, top))[None], 50.0, colors=colors, background=(0.2, 0.4, 0.6), **FLAT)
        assert (seg == n - 1).any() and len(set(seg[seg >= 0].tolist()) - {n - 1}) >= 5 and (rgb[seg < 0] == [51, 102, 153, 0]).all() and np.array_equal(rgb.reshape(-1, 4), _flat(seg, colors, (0.2, 0.4, 0.6)))
        assert (nrm[seg < 0] == 0).all() and (depth[seg < 0] == -1).all() and np.allclose(np.linalg.norm(nrm[seg >= 0], axis=1), 1.0, atol=1e-5)


def test_named_camera_default_colours_mask_and_out():
    """camera_cases.XML, the ball coloured, a material on the post: colors=None paints info["geom_rgba"]; masked worlds keep their bytes in out= and read background, depth -1, normal 0 in fresh tensors"""
    import torch
    model = C.compile_xml(K.XML.replace('name="ball"', 'name="ball" rgba="0.9 0.1 0.2 1"').replace('name="post"', 'name="post" material="wood"').replace(
        "<worldbody>", '<asset><material name="wood" rgba="0.6 0.4 0.2 1"/></asset><worldbody>'))
    with contextlib.closing(_sim(model, 5, C.f32(np.array([[0.0], [0.7], [-1.1], [1.2], [3.0]])), np.zeros((5, 1)))) as sim:
        sim.forward()
        mask, kw, on, off = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8, device=sim.device), dict(background=(1.0, 0.0, 0.5), **FLAT), [0, 2], [1, 3, 4]
        depth, seg, rgb, nrm = _images(sim.render, sim, 1, 16, 16, "overview", mask=mask, **kw)
        assert {sim.geom_id("ball"), sim.geom_id("post"), sim.geom_id("floor")} <= set(seg[on].ravel().tolist()) and np.array_equal(rgb[on].reshape(-1, 4), _flat(seg[on], np.asarray(model.info["geom_rgba"])[:, :3], kw["background"]))
        assert (rgb[off] == BYTE).all() and np.isnan(nrm[off]).all() and np.isnan(depth[off]).all() and (seg[off] == SENTINEL).all()
        fresh = [x.cpu().numpy() for x in sim.render("overview", 16, 16, rgb=True, normals=True, mask=mask, **kw)]
        assert (fresh[0][off] == -1.0).all() and fresh[1].dtype == np.uint8 and (fresh[1][off] == [255, 0, 128, 0]).all() and (fresh[2][off] == 0).all() and len(fresh) == 3 and all(np.array_equal(x[on], y[on]) for x, y in zip(fresh, (depth, rgb, nrm)))


REFUSALS = [("null model", dict(m=None)), ("null camera block", dict(block=False)), ("null shade block", dict(shade=False)),
            ("null rgba and normal", dict(rgba=None, normal=None)), ("rgba without colors", dict(colors=None)), ("null camera poses", dict(pose_pos=None)),
            ("outside 1 .. 1024", dict(w=1025)), ("finite and >= 0", dict(ambient=-0.1)), ("finite and >= 0", dict(diffuse=float("nan"))),
            ("finite and >= 0", dict(sun_diffuse=float("inf"))), ("sun is zero", dict(sun=(0.0, 0.0, 0.0))), ("sun is zero", dict(sun=(float("nan"), 0.0, 1.0))),
            ("background is not finite", dict(background=(0.0, float("inf"), 0.0)))]


@pytest.mark.parametrize("word, kw", REFUSALS)
def test_c_abi_refusals(crowd, word, kw):
    """-1 with a message, before anything is launched: over full blocks (two posed cameras, 4 x 4) with one thing wrong, the images stay zero"""
    import torch
    sim, vec = crowd[0], lambda x: (ctypes.c_float * len(x))(*x) if isinstance(x, tuple) else x
    out, fovy = torch.zeros((5, sim.num_worlds, 2, 4, 4, 9), device=sim.device), vec((45.0, 45.0))      # slabs: depth, rgba, normal, (zero) poses, (zero) colours
    cam = dict(xpos=sim.xpos.data_ptr(), xquat=sim.xquat.data_ptr(), pose_pos=out[3].data_ptr(), pose_mat=out[3].data_ptr(), cam_fovy=ctypes.addressof(fovy), depth=out[0].data_ptr())
    shade = dict(rgba=out[1].data_ptr(), normal=out[2].data_ptr(), colors=out[4].data_ptr(), ambient=0.3, diffuse=0.7, sun=(0.0, 0.0, -1.0), sun_diffuse=0.5, background=(0.0, 0.0, 0.0))
    b, s = _native.SimCamerasStruct(**{f: kw.get(f, v) for f, v in cam.items()}), _native.SimShadeStruct(**{f: vec(kw.get(f, v)) for f, v in shade.items()})
    rc = sim._L.grx_sim_render_rgb(kw.get("m", sim._h), ctypes.byref(b) if kw.get("block", True) else None, ctypes.byref(s) if kw.get("shade", True) else None, sim.num_worlds, 2, 4, kw.get("w", 4), None)
    torch.cuda.synchronize()
    assert rc == -1 and word in sim._L.grx_last_error().decode() and not out.any(), sim._L.grx_last_error()
