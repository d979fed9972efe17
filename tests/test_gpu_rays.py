"""Ray casting on the device: BatchedSim.ray / ray_sites / rangefinder and the C ABI's error returns, against the fp64 reference of tests/ray_cases.py under its
acceptance rule (which rays are compared is decided by the reference alone).  The outputs are filled with NaN / a sentinel before every launch: an element the launch
does not write fails the finiteness check."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

import engine_matrix_cases as C
import ray_cases as R
import sim_cases as S

pytestmark = pytest.mark.gpu
SENTINEL = -77


def _sim(model, n, q0, v0, outputs=("xpos", "xquat"), ctrl=None):
    import torch

    import gymnasium_robotics_amd as grx

    assert torch.cuda.is_available(), "these tests need the GPU"
    sim = grx.BatchedSim(model, num_worlds=n, outputs=outputs)
    for k, rows in (("qpos", q0), ("qvel", v0)) + ((("ctrl", ctrl),) if ctrl is not None else ()):
        getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).reshape(getattr(sim, k).shape))
    sim.qacc_warmstart.zero_()
    return sim


def _filled(sim, n_rays):
    import torch

    return (torch.full((sim.num_worlds, n_rays), float("nan"), device=sim.device), torch.full((sim.num_worlds, n_rays), SENTINEL, dtype=torch.int32, device=sim.device))


def _cast(sim, o, d, **kw):
    """sim.ray into NaN / sentinel-filled outputs; host arrays back"""
    import torch

    out = _filled(sim, o.shape[1])
    dist, geom = sim.ray(torch.from_numpy(np.ascontiguousarray(o, dtype=np.float32)).to(sim.device), torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).to(sim.device), out=out, **kw)
    assert dist is out[0] and geom is out[1]
    torch.cuda.synchronize()
    return dist.cpu().numpy(), geom.cpu().numpy()


@pytest.fixture(scope="module")
def crowd():
    """per variant of crowd-mixed (5 and 13 worlds) a simulation after forward() on the start states, and its worlds' reference"""
    made = {}

    def get(variant):
        if variant not in made:
            var = R.M.group(R.SCENE).variants[variant]
            sim = _sim(var.model, len(var.idx), var.q0, var.v0)
            sim.forward()
            made[variant] = (sim, [R.world(variant, i) for i in range(len(var.idx))])
        return made[variant]

    yield get
    for sim, _ in made.values():
        sim.close()


@pytest.mark.parametrize("n_rays", [1, 3, 64, 65, 130])
def test_ray_against_the_reference_five_worlds(crowd, n_rays):
    """the wave and workgroup edges of the launch shape: 64 worlds per wave (R = 1), a ragged group (3), one wave per world (64), one ray past it (65), a partial block (130)"""
    sim, worlds = crowd(0)
    o, d = (np.stack([getattr(w, k)[:n_rays] for w in worlds]) for k in ("o", "d"))
    dist, geom = _cast(sim, o, d)
    for i, w in enumerate(worlds):
        R.accept(("mi355x", n_rays, i), w.model, dist[i], geom[i], w.dist[:n_rays], w.geom[:n_rays], w.compared[:n_rays], {})


def test_ray_against_the_reference_thirteen_worlds(crowd):
    sim, worlds = crowd(1)
    worst = {}
    o, d = (np.stack([getattr(w, k) for w in worlds]) for k in ("o", "d"))
    dist, geom = _cast(sim, o, d)
    for i, w in enumerate(worlds):
        R.accept(("mi355x", 13, i), w.model, dist[i], geom[i], w.dist, w.geom, w.compared, worst)
    sim5, worlds5 = crowd(0)
    dist, geom = _cast(sim5, *(np.stack([getattr(w, k) for w in worlds5]) for k in ("o", "d")))
    for i, w in enumerate(worlds5):
        R.accept(("mi355x", 5, i), w.model, dist[i], geom[i], w.dist, w.geom, w.compared, worst)
    print("worst error per type", worst)
    assert set(worst) == set(R.TYPE_NAMES.values())
    R.record("mi355x", worst)


def _filtered(crowd, kw_ref, kw_sim, extra=None):
    sim, worlds = crowd(0)
    o, d = (np.stack([getattr(w, k) for w in worlds]) for k in ("o", "d"))
    if extra is not None:
        o, d = extra(worlds, o, d)
    dist, geom = _cast(sim, o, d, **kw_sim)
    changed = 0
    for i, w in enumerate(worlds):
        want_dist, want_geom = R.cast(w.model, w.gxpos, w.gxmat, o[i], d[i], **kw_ref)
        free_dist, free_geom = R.cast(w.model, w.gxpos, w.gxmat, o[i], d[i])
        compared = R.compared_mask(w.model, w.gxpos, w.gxmat, o[i], d[i], want_dist, want_geom, (w.index, 2), **kw_ref)
        R.accept(("mi355x", str(kw_ref), i), w.model, dist[i], geom[i], want_dist, want_geom, compared, {})
        assert compared.mean() >= R.MIN_SHARE, (i, compared.mean())
        changed += int((compared & (want_geom != free_geom)).sum())
    assert changed >= 5, "the filter changes too few compared rays of this set to test anything"


def test_exclude_body_with_a_ray_that_starts_inside_the_excluded_geom(crowd):
    """body 4's geom is skipped by every ray; ray 0 of every world starts at that geom's centre and must see what lies beyond it (or nothing), never the geom itself"""
    sim, worlds = crowd(0)
    G = R.geoms_of(worlds[0].model)
    g = int(np.nonzero(G.body == 4)[0][0])

    def extra(worlds, o, d):
        for i, w in enumerate(worlds):
            o[i, 0], d[i, 0] = C.f32(w.gxpos[g]), [0.3, 0.2, -1.0]
        return o, d

    _filtered(crowd, dict(exclude_body=4), dict(exclude_body=4), extra)
    o, d = extra(worlds, *(np.stack([getattr(w, k) for w in worlds]) for k in ("o", "d")))
    _, geom = _cast(sim, o, d, exclude_body=[4] + [-1] * (R.RAYS - 1))
    assert (geom[:, 0] != g).all() and (geom[:, 0] >= 0).all()
    _, geom = _cast(sim, o, d)
    assert (geom[:, 0] == g).all()      # without the filter the ray leaves through the geom it starts in


def test_include_static_off(crowd):
    _filtered(crowd, dict(include_static=False), dict(include_static=False))


def test_max_dist(crowd):
    _filtered(crowd, dict(max_dist=0.5), dict(max_dist=0.5))


def test_masked_rows_keep_their_bits(crowd):
    import torch

    sim, worlds = crowd(0)
    o, d = (np.stack([getattr(w, k) for w in worlds]) for k in ("o", "d"))
    mask = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8, device=sim.device)
    dist, geom = _cast(sim, o, d, mask=mask)
    assert np.isnan(dist[[1, 3, 4]]).all() and (geom[[1, 3, 4]] == SENTINEL).all()
    fresh_dist, fresh_geom = sim.ray(torch.from_numpy(o.astype(np.float32)).to(sim.device), torch.from_numpy(d.astype(np.float32)).to(sim.device), mask=mask)
    torch.cuda.synchronize()      # without out=: the rows of the worlds the mask leaves out read "no hit", the others are the launch's
    assert (fresh_dist.cpu().numpy()[[1, 3, 4]] == -1.0).all() and (fresh_geom.cpu().numpy()[[1, 3, 4]] == -1).all()
    assert np.array_equal(fresh_dist.cpu().numpy()[[0, 2]], dist[[0, 2]]) and np.array_equal(fresh_geom.cpu().numpy()[[0, 2]], geom[[0, 2]])
    for i in (0, 2):
        w = worlds[i]
        R.accept(("mi355x", "mask", i), w.model, dist[i], geom[i], w.dist, w.geom, w.compared, {})
        assert w.compared.mean() >= R.MIN_SHARE


@pytest.fixture(scope="module")
def arm():
    scene = S.SCENES["arm"]
    st = scene.states(S.N_WORLDS)
    sim = _sim(scene.model, S.N_WORLDS, st["qpos"], st["qvel"], outputs=("xpos", "xquat", "site_xpos", "site_xmat"), ctrl=st["ctrl"])
    yield scene, st, sim
    sim.close()


def _arm_reference(scene, st, nstep):
    """per world the oracle's geom poses after step(nstep) (0: forward) -- after a step the ones of the last substep's position stage, which is what MjData holds"""
    out = []
    for i in range(S.N_WORLDS):
        S.oracle_world(scene, st, i, nstep)
        orc = S._oracle(scene)
        out.append((orc.geom_xpos.reshape(-1, 3).copy(), orc.geom_xmat.reshape(-1, 9).copy(), orc.site_xpos.reshape(-1, 3).copy(), orc.site_xmat.reshape(-1, 3, 3).copy()))
    return out


def test_ray_sites_is_ray_fed_with_the_site_frames(arm):
    """geoms equal, dist within the bound: the same rays built by torch from site_xpos / site_xmat; and the rays that exclude the site's own body against the reference"""
    import torch

    scene, st, sim = arm
    sim.forward()
    rng = np.random.default_rng(5)
    sites = ["ee", "pad"] * 32
    local = torch.from_numpy(C.f32(rng.standard_normal((64, 3))).astype(np.float32)).to(sim.device)
    ids = torch.tensor([sim.site_id(s) for s in sites], device=sim.device)
    o = sim.site_xpos[:, ids]
    d = (sim.site_xmat[:, ids].view(sim.num_worlds, 64, 3, 3) @ local[None, :, :, None]).squeeze(-1)
    own = torch.tensor([int(np.asarray(scene.model.tables["site_bodyid"]).reshape(-1)[sim.site_id(s)]) for s in sites], dtype=torch.int32, device=sim.device)
    for own_body in (False, True):
        out = _filled(sim, 64)
        a_dist, a_geom = sim.ray_sites(sites, local, exclude_own_body=own_body, out=out)
        b_dist, b_geom = sim.ray(o, d, exclude_body=own if own_body else None, out=_filled(sim, 64))
        torch.cuda.synchronize()
        a_dist, a_geom, b_dist, b_geom = (x.cpu().numpy() for x in (a_dist, a_geom, b_dist, b_geom))
        assert np.isfinite(a_dist).all() and (a_geom == b_geom).all()
        assert (a_geom >= 0).sum() >= 20 and (a_geom < 0).sum() >= 20      # hits and misses are both there to be compared
        assert (np.abs(a_dist - b_dist) <= C.BOUND * np.maximum(1.0, np.abs(b_dist))).all()
    ref = _arm_reference(scene, st, 0)
    for i, (gx, gm, sx, sm) in enumerate(ref):
        ro, rd = sx[ids.cpu().numpy()], np.einsum("rij,rj->ri", sm[ids.cpu().numpy()], local.cpu().numpy().astype(np.float64))
        kw = dict(exclude_body=own.cpu().numpy())
        want_dist, want_geom = R.cast(scene.model, gx, gm, ro, rd, **kw)
        compared = R.compared_mask(scene.model, gx, gm, ro, rd, want_dist, want_geom, (i, 3), **kw)
        R.accept(("mi355x", "ray_sites", i), scene.model, a_dist[i], a_geom[i], want_dist, want_geom, compared, {})
        assert compared.mean() >= R.MIN_SHARE, (i, compared.mean())


def test_rays_after_a_step_see_the_stale_poses(arm):
    """after step(4) the rays are cast against the xpos / xquat the launch wrote: MjData's geom_xpos of the last substep's position stage, the oracle's after its step(4)"""
    scene, st, sim = arm
    import torch

    for k in ("qpos", "qvel", "ctrl"):
        getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)).reshape(getattr(sim, k).shape))
    sim.qacc_warmstart.zero_()
    sim.step(4)
    ref = _arm_reference(scene, st, 4)
    rays = [R.make_rays(scene.model, gx, 1000 + i, min_up=0.6) for i, (gx, _, _, _) in enumerate(ref)]      # half of the aimed rays go to the floor here: none at a shallow angle
    o, d = np.stack([r[0] for r in rays]), np.stack([r[1] for r in rays])
    dist, geom = _cast(sim, o, d)
    share = []
    for i, (gx, gm, _, _) in enumerate(ref):
        want_dist, want_geom = R.cast(scene.model, gx, gm, o[i], d[i])
        compared = R.compared_mask(scene.model, gx, gm, o[i], d[i], want_dist, want_geom, (i, 4))
        R.accept(("mi355x", "step4", i), scene.model, dist[i], geom[i], want_dist, want_geom, compared, {})
        share.append(compared.mean())
    assert min(share) >= R.MIN_SHARE, share


def _grid_xml(n_boxes):
    cols = int(np.ceil(np.sqrt(n_boxes)))
    boxes = "".join(f'<geom type="box" size="0.04 0.04 {0.02 + 0.001 * (k % 7)}" pos="{0.12 * (k % cols)} {0.12 * (k // cols)} 0.05"/>' for k in range(n_boxes))
    return f'<mujoco><worldbody>{boxes}<body pos="-1 -1 1"><freejoint/><geom type="sphere" size="0.05" mass="1"/></body></worldbody></mujoco>'


@pytest.mark.parametrize("n_rays, over", [(1, 0), (1, 1), (64, 0), (64, 1)])
def test_one_geom_more_than_a_tile(n_rays, over):
    """static boxes in a grid and a free sphere, as many geoms as a tile of the launch holds (7 for R = 1, 127 for R = 64: the launch shape says) and one more: the last
    geoms sit at the end of the tile or alone in a second one, and every world aims at them"""
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import emu_rays

    gtile = emu_rays.shape(n_rays)[3]
    n_boxes = gtile - 1 + over      # the sphere is one more geom

    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "grid.xml")
        with open(p, "w") as fh:
            fh.write(_grid_xml(n_boxes))
        from gymnasium_robotics_amd.mjcf import compile_mjcf

        model = compile_mjcf(p)
    from oracle.oracle_sim import OracleSim

    orc = OracleSim(model)
    orc.forward()
    gx, gm = orc.geom_xpos.reshape(-1, 3).copy(), orc.geom_xmat.reshape(-1, 9).copy()
    n = 5
    assert len(gx) == gtile + over
    sim = _sim(model, n, np.tile(orc.qpos, (n, 1)), np.zeros((n, orc.nv)))
    try:
        sim.forward()
        rng = np.random.default_rng(n_boxes)
        o, d = np.zeros((n, n_rays, 3)), np.zeros((n, n_rays, 3))
        for i in range(n):
            for r in range(n_rays):
                g = (len(gx) - 1 - i - r) % len(gx)      # from the last geom backwards: ray 0 of world 0 aims at the last one
                o[i, r] = gx[g] + np.r_[0.01 * rng.standard_normal(2), 0.6]
                d[i, r] = np.r_[0.01 * rng.standard_normal(2), -1.0]
        o, d = C.f32(o), C.f32(d)
        dist, geom = _cast(sim, o, d)
        hit_last = 0
        for i in range(n):
            want_dist, want_geom = R.cast(model, gx, gm, o[i], d[i])
            compared = R.compared_mask(model, gx, gm, o[i], d[i], want_dist, want_geom, (i, n_boxes))
            R.accept(("mi355x", "grid", n_boxes, i), model, dist[i], geom[i], want_dist, want_geom, compared, {})
            assert compared.all()
            hit_last += int((geom[i] >= len(gx) - 2).sum())
        assert hit_last >= 2
    finally:
        sim.close()


RF_XML = """<mujoco><worldbody>
  <geom name="floor" type="plane" size="2 2 0.1"/>
  <geom name="wall" type="box" size="0.05 1 1" pos="1.0 0 1"/>
  <body name="a" pos="0 0 0.8"><freejoint/><geom name="ball" type="sphere" size="0.1" mass="1"/>
    <site name="down" pos="0 0 0" quat="0 1 0 0"/><site name="side" pos="0 0 0" quat="0.7071067811865476 0 0.7071067811865476 0"/></body>
</worldbody><sensor><rangefinder name="height" site="down"/><rangefinder name="ahead" site="side" cutoff="0.5"/><rangefinder name="far" site="side" cutoff="2"/></sensor></mujoco>"""


def test_rangefinder_readings_and_cutoff():
    """sites at the ball's centre: the site's own body is excluded, so `height` reads the floor (0.8 + the world's lift), `ahead` sees the wall at 0.95 m, beyond its cutoff of
    0.5 (-1), `far` reads it"""
    import torch

    import gymnasium_robotics_amd as grx

    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "rf.xml")
        with open(p, "w") as fh:
            fh.write(RF_XML)
        sim = grx.BatchedSim(p, 5, outputs=("xpos", "xquat", "site_xpos", "site_xmat"))
    try:
        lift = torch.tensor([0.0, 0.1, 0.2, 0.3, 0.4], device=sim.device)
        sim.reset()
        sim.qpos[:, 2] += lift
        sim.forward()
        got = sim.rangefinder()
        torch.cuda.synchronize()
        got, lift = got.cpu().numpy().astype(np.float64), lift.cpu().numpy().astype(np.float64)
        assert got.shape == (5, 3) and sim.rangefinder_id("ahead") == 1
        assert np.abs(got[:, 0] - (0.8 + lift)).max() < C.BOUND * 1.2 and (got[:, 1] == -1.0).all() and np.abs(got[:, 2] - 0.95).max() < C.BOUND
        keep = sim.rangefinder(mask=[1, 1, 0, 1, 1])
        torch.cuda.synchronize()
        assert np.abs(keep.cpu().numpy()[[0, 1, 3, 4]] - got[[0, 1, 3, 4]]).max() == 0
        assert (keep.cpu().numpy()[2] == -1.0).all()      # the world the mask leaves out reads "no reading"
    finally:
        sim.close()


def test_c_abi_error_returns(arm):
    from gymnasium_robotics_amd import _native

    scene, st, sim = arm
    sim.forward()
    L, h = sim._L, sim._h
    out = _filled(sim, 2)
    zeros = np.zeros((sim.num_worlds, 2, 3), np.float32)
    import torch

    o = torch.from_numpy(zeros).to(sim.device)
    full = dict(xpos=sim.xpos.data_ptr(), xquat=sim.xquat.data_ptr(), origin=o.data_ptr(), direction=o.data_ptr(), site_xpos=sim.site_xpos.data_ptr(), site_xmat=sim.site_xmat.data_ptr(),
                local_dir=o.data_ptr(), dist=out[0].data_ptr(), geom=out[1].data_ptr(), include_static=1)
    sites = (ctypes.c_int * 2)(0, 1)
    block = lambda **kw: _native.SimRaysStruct(**{**full, "ray_site": ctypes.cast(sites, ctypes.c_void_p).value, **kw})

    def refused(fn, m, b, n, r, word):
        assert fn(m, None if b is None else ctypes.byref(b), n, r, None) == -1
        assert word in L.grx_last_error().decode(), L.grx_last_error()

    for fn in (L.grx_sim_ray, L.grx_sim_ray_sites):
        refused(fn, None, block(), 5, 2, "null model")
        refused(fn, h, None, 5, 2, "null ray block")
        refused(fn, h, block(xpos=None), 5, 2, "null body poses")
        refused(fn, h, block(xquat=None), 5, 2, "null body poses")
        refused(fn, h, block(dist=None), 5, 2, "null dist")
        refused(fn, h, block(), 0, 2, "n_worlds < 1")
        refused(fn, h, block(), 5, 0, "n_rays < 1")
    refused(L.grx_sim_ray, h, block(origin=None), 5, 2, "null origin")
    refused(L.grx_sim_ray_sites, h, block(site_xmat=None), 5, 2, "null site poses")
    refused(L.grx_sim_ray_sites, h, block(local_dir=None), 5, 2, "null ray_site / local_dir")
    for bad in (-1, sim.nsite):
        sites[1] = bad
        refused(L.grx_sim_ray_sites, h, block(), 5, 2, "outside [0, nsite)")
    sites[1] = 1
    assert L.grx_sim_ray_sites(h, ctypes.byref(block(geom=None)), 5, 2, None) == 0      # geom is optional; a zero direction is a miss, never a fault
    torch.cuda.synchronize()
    assert (out[0].cpu().numpy() == -1.0).all() and (out[1].cpu().numpy() == SENTINEL).all()
    with tempfile.TemporaryDirectory() as tmp:      # a model compiled with an origin is refused, as by grx_sim_step
        p = os.path.join(tmp, "arm.xml")
        with open(p, "w") as fh:
            fh.write(S.ARM_XML)
        from gymnasium_robotics_amd.mjcf import compile_mjcf

        shifted = compile_mjcf(p, origin=[0.5, 0.0, 0.0], **scene.compile_kwargs)
    H, I, F = shifted.pack()
    hs = _native.acquire_model(H, I, F, sim.device.index or 0)
    try:
        refused(L.grx_sim_ray, hs, block(), 5, 2, "compiled with an origin")
    finally:
        _native.release_model(hs)
    # a mesh that meets planes only has no full hull in the compiled model: refused by geom id before anything is launched
    rock = C.compile_xml('<mujoco><asset><mesh name="ico12" file="ico12.stl"/></asset><worldbody><geom type="plane" size="2 2 0.1"/>'
                         '<body pos="0 0 0.5"><freejoint/><geom type="mesh" mesh="ico12" mass="1"/></body></worldbody></mujoco>')
    H, I, F = rock.pack()
    hr = _native.acquire_model(H, I, F, sim.device.index or 0)
    try:
        refused(L.grx_sim_ray, hr, block(), 5, 2, "geom 1 is a mesh without a full hull")
    finally:
        _native.release_model(hr)
