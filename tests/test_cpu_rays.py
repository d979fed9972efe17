"""Ray casting on the CPU: the routines of csrc/grx_rays.h compiled for the host (tests/emu/emu_rays.py) against the fp64 reference of tests/ray_cases.py, the reference
against its independent route, the derived hull planes against scipy's, and the bookkeeping around them (the launch shape, the C ABI's layout, the compiler's rangefinders)."""
import ctypes
import os
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rays  # noqa: E402
import engine_matrix_cases as C  # noqa: E402
import ray_cases as R  # noqa: E402

WORLDS = [(v, i) for v in (0, 1) for i in range(R.M.CROWD_WORLDS[v])]


@pytest.fixture(scope="module")
def emu():
    return emu_rays.RayEmu(R.world(0, 0).model)


def test_reference_agrees_with_the_inside_functions():
    for key in ((0, 0), (1, 12)):
        w = R.world(*key)
        R.check_reference(w.model, w.gxpos, w.gxmat, w.o, w.d, w.dist, w.geom)


def test_host_routines_against_the_reference_on_crowd_mixed(emu):
    """every world of the scene: at least 90 % of its rays are compared (the reference alone decides), the compared rays agree, and over the scene every one of the seven
    geom types is the hit geom of at least 20 compared rays; the ray sets hold inside starts, rays leaving the plane, misses, a zero and a NaN direction"""
    worst, hits = {}, {}
    for v, i in WORLDS:
        w = R.world(v, i)
        assert w.compared.mean() >= R.MIN_SHARE, (v, i, "share of compared rays", w.compared.mean())
        dist, geom = emu.cast(w.xpos, w.xquat, w.o, w.d)
        assert dist[-1] == -1 and geom[-1] == -1 and dist[-2] == -1 and geom[-2] == -1      # the NaN and the zero direction
        R.accept(("host", v, i), w.model, dist, geom, w.dist, w.geom, w.compared, worst)
        G = R.geoms_of(w.model)
        for r in np.nonzero(w.compared & (w.geom >= 0))[0]:
            name = R.TYPE_NAMES[int(G.type[w.geom[r]])]
            hits[name] = hits.get(name, 0) + 1
        assert (w.geom == -1).sum() >= 8 and (w.compared & (w.geom == -1)).sum() >= 8      # misses are compared too
    print("compared hits per type", hits, "worst error per type", worst)
    assert set(hits) == set(R.TYPE_NAMES.values()) and min(hits.values()) >= 20, hits
    R.record("host", worst)


def test_inside_starts_leave_through_the_far_side():
    """a ray that starts inside a solid reports the exit point: its hit geom is the solid it started in, for every solid type"""
    w = R.world(0, 1)
    G = R.geoms_of(w.model)
    seen = set()
    for r in range(R.RAYS):
        if w.geom[r] < 0 or G.type[w.geom[r]] == 0:
            continue
        g = w.geom[r]
        f0 = R.inside_f(G.type[g], G.size[g], G.planes.get(g), ((w.o[r] - w.gxpos[g]) @ w.gxmat[g].reshape(3, 3))[None])[0]
        if f0 < 0:
            seen.add(R.TYPE_NAMES[int(G.type[g])])
    assert seen == set(R.TYPE_NAMES.values()) - {"plane"}, seen


@pytest.mark.parametrize("kw", [dict(exclude_body=3), dict(include_static=False), dict(max_dist=0.6), dict(exclude_body=5, include_static=False, max_dist=1.0)], ids=str)
def test_filters_on_the_host(emu, kw):
    w = R.world(1, 3)
    want_dist, want_geom = R.cast(w.model, w.gxpos, w.gxmat, w.o, w.d, **kw)
    compared = R.compared_mask(w.model, w.gxpos, w.gxmat, w.o, w.d, want_dist, want_geom, (w.index, 1), **kw)
    dist, geom = emu.cast(w.xpos, w.xquat, w.o, w.d, **kw)
    R.accept(("host", str(kw)), w.model, dist, geom, want_dist, want_geom, compared, {})
    assert compared.mean() >= R.MIN_SHARE, compared.mean()
    base = R.world(1, 3)
    assert (want_geom != base.geom).any(), "the filter changes no ray of this set"


def test_tiles_give_the_same_answer(emu):
    w = R.world(0, 2)
    whole = emu.cast(w.xpos, w.xquat, w.o, w.d)
    for gtile in (1, 5, 8, 17, 18):
        part = emu.cast(w.xpos, w.xquat, w.o, w.d, gtile=gtile)
        assert (part[0] == whole[0]).all() and (part[1] == whole[1]).all(), gtile


@pytest.mark.parametrize("mesh", C.MESHES)
def test_derived_hull_planes_against_scipy(mesh):
    """same face count after merging, every plane within 1e-6 of one of scipy's and the other way round"""
    model = R.world(0, 0).model
    G = R.geoms_of(model)
    nvert = {"ico12": 12, "ico42": 42}[mesh]
    g = next(g for g in G.verts if len(G.verts[g]) == nvert)
    mine, ref = emu_rays.hull_planes(model, g).astype(np.float64), G.planes[g]
    assert len(mine) == len(ref) == {"ico12": 20, "ico42": 80}[mesh]
    d = np.abs(mine[:, None, :] - ref[None, :, :]).max(axis=2)
    assert d.min(axis=1).max() < 1e-6 and d.min(axis=0).max() < 1e-6, (d.min(axis=1).max(), d.min(axis=0).max())


def _solid(kind, rng):
    """vertices of a box or of a hexagonal prism (flat faces of 4 and 6 vertices) in general orientation, about their centre"""
    if kind == "box":
        v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * rng.uniform(0.02, 0.3, 3)
    else:
        ang = np.arange(6) * np.pi / 3 + rng.uniform(0, 1)
        ring = np.stack([np.cos(ang), np.sin(ang)], axis=1) * rng.uniform(0.02, 0.3)
        h = rng.uniform(0.02, 0.3)
        v = np.array([[x, y, z] for z in (-h, h) for x, y in ring])
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    return np.array([C.quat_rot(q, p) for p in v]) + rng.uniform(-0.5, 0.5, 3)


@pytest.mark.parametrize("kind, faces", [("box", 6), ("prism", 8)])
def test_derived_hull_planes_of_flat_faced_solids(kind, faces):
    """the compiler's path for a mesh with flat faces of more than three vertices: the adjacency comes from a triangulation of the fp64 vertices (one diagonal per quad,
    chosen there), the handle holds the vertices rounded to fp32, which folds such a face by about 1e-8 of the extent, either way.  Every solid keeps all its faces, the
    planes are scipy's within 1e-5 of the extent, every vertex is inside every plane, and a ray from the centre leaves through a face in every direction at the exact
    solid's distance: the hull is closed"""
    from scipy.spatial import ConvexHull

    rng = np.random.default_rng(11 if kind == "box" else 12)
    for case in range(200):
        v64 = _solid(kind, rng)
        hull = ConvexHull(v64)
        adj = [set() for _ in v64]
        for tri in hull.simplices:
            for a, b in ((0, 1), (1, 2), (2, 0)):
                adj[tri[a]].add(int(tri[b]))
                adj[tri[b]].add(int(tri[a]))
        centred = v64 - v64.mean(axis=0)
        v32 = centred.astype(np.float32).astype(np.float64)
        mine = emu_rays.planes_of(v32, [sorted(a) for a in adj]).astype(np.float64)
        ref = R.scipy_planes(centred)
        ref = np.array([p for k, p in enumerate(ref) if not any(np.abs(p - q).max() < 1e-7 for q in ref[:k])])      # the triangles of a face, merged
        ext = np.abs(v32).max()
        assert len(ref) == faces and len(mine) == faces, (kind, case, len(mine))
        dmat = np.abs(mine[:, None, :] - ref[None, :, :]).max(axis=2)
        assert dmat.min(axis=1).max() < 1e-5 * max(ext, 1.0) and dmat.min(axis=0).max() < 1e-5 * max(ext, 1.0), (kind, case)
        assert (v32 @ mine[:, :3].T - mine[:, 3]).max() <= 1e-7 * ext, (kind, case, "a vertex outside a plane")
        for _ in range(20):
            d = rng.standard_normal(3)
            want = R.geom_hits(7, None, ref, np.zeros((1, 3)), d[None])[0]
            got = emu_rays.planes_hit(np.zeros(3), d, mine)
            assert np.isfinite(want) and got > 0 and abs(got - want) <= 1e-5 * max(1.0, want), (kind, case, got, want)


MESH_ON_A_PLANE = """<mujoco><asset><mesh name="ico12" file="ico12.stl"/></asset><worldbody><geom name="floor" type="plane" size="2 2 0.1"/>
  <body pos="0 0 0.5"><freejoint/><geom name="rock" type="mesh" mesh="ico12" mass="1"/></body></worldbody></mujoco>"""


def test_a_mesh_without_a_full_hull_is_refused_by_name():
    """a mesh that meets planes only keeps no full hull in the compiled model; the ray calls say so rather than cast through it"""
    from gymnasium_robotics_amd.sim import BatchedSim

    model = C.compile_xml(MESH_ON_A_PLANE)
    g = model.names["geom"]["rock"]
    assert int(np.asarray(model.tables["geom_type"]).reshape(-1)[g]) == 7 and int(np.asarray(model.tables["geom_hullnum"]).reshape(-1)[g]) == 0
    sim = BatchedSim(model, 2, outputs=("xpos", "xquat", "site_xpos", "site_xmat"))
    with pytest.raises(ValueError, match="rock"):
        sim.ray(np.zeros((1, 3)), np.ones((1, 3)))
    with pytest.raises(ValueError, match="rock"):
        sim.ray_sites([], np.ones((1, 3)))
    crowd = BatchedSim(R.world(0, 0).model, 2, outputs=("xpos", "xquat"))
    crowd._ray_need("ray()", ("xpos", "xquat"))      # every mesh of crowd-mixed has a convex partner


def test_launch_shape():
    """lanes cover (worlds of the group) x (rays of the chunk); the staging area holds the group's tiles; a one-ray launch packs 64 worlds into a wave"""
    for n in (1, 2, 3, 16, 63, 64, 65, 128, 130, 255, 256, 257, 1000):
        rpb, wpb, threads, gtile, stride = emu_rays.shape(n)
        assert rpb == min(n, 256) and 1 <= wpb <= 64 and wpb * rpb <= threads <= 256 and threads % 64 == 0 and gtile >= 1, (n, rpb, wpb, threads, gtile)
        assert stride >= 20 * gtile and wpb * stride <= 512 * 20, (n, wpb, gtile, stride)      # the worlds' tiles lie side by side inside the staging area
        assert wpb == 1 or stride % 2 == 1, (n, stride)      # an odd stride: the worlds of a wave read different LDS banks
    assert emu_rays.shape(1) == (1, 64, 64, 7, 141) and emu_rays.shape(64)[1:4] == (4, 256, 127) and emu_rays.shape(256)[1:] == (1, 256, 512, 10240)


def test_c_abi_layout_and_symbols():
    from gymnasium_robotics_amd import _native

    L = _native.lib()
    assert {"grx_sim_ray", "grx_sim_ray_sites", "grx_sim_rays_layout"} <= set(_native.EXPORTED_SYMBOLS) and all(hasattr(L, s) for s in ("grx_sim_ray", "grx_sim_ray_sites"))
    n = L.grx_sim_rays_layout(None, 0)
    out = (ctypes.c_longlong * n)()
    assert L.grx_sim_rays_layout(out, n) == n == 1 + len(_native.SimRaysStruct._fields_)
    assert out[0] == ctypes.sizeof(_native.SimRaysStruct)
    assert [out[1 + k] for k in range(n - 1)] == [getattr(_native.SimRaysStruct, f).offset for f, _ in _native.SimRaysStruct._fields_]
    b = _native.SimRaysStruct()
    assert L.grx_sim_ray(None, ctypes.byref(b), 1, 1, None) == -1 and b"null model" in L.grx_last_error()


def test_a_rangefinder_without_a_site_compiles_and_is_reported_when_read():
    from gymnasium_robotics_amd.mjcf import compile_mjcf
    from gymnasium_robotics_amd.sim import BatchedSim

    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "rf.xml")
        with open(p, "w") as fh:
            fh.write(RF_XML.replace('<rangefinder name="height" site="down"/>', '<rangefinder name="height"/>'))
        model = compile_mjcf(p)
    assert model.info["rangefinder"][0] == dict(site=None, cutoff=0.0)
    with pytest.raises(ValueError, match="height"):
        BatchedSim(model, 2, outputs=("xpos", "xquat", "site_xpos", "site_xmat")).rangefinder()


RF_XML = """<mujoco><worldbody>
  <geom name="floor" type="plane" size="2 2 0.1"/>
  <body name="a" pos="0 0 1"><freejoint/><geom type="sphere" size="0.1" mass="1"/><site name="down" pos="0 0 -0.2" quat="0 1 0 0"/><site name="side" pos="0.2 0 0" quat="0.7071068 0 0.7071068 0"/></body>
</worldbody><sensor><rangefinder name="height" site="down"/><touch name="t" site="side"/><rangefinder site="side" cutoff="0.5"/><rangefinder name="again" site="down" cutoff="3"/></sensor></mujoco>"""


def test_compiler_records_the_rangefinders():
    from gymnasium_robotics_amd.mjcf import compile_mjcf
    from gymnasium_robotics_amd.sim import BatchedSim

    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "rf.xml")
        with open(p, "w") as fh:
            fh.write(RF_XML)
        full, cut = compile_mjcf(p), compile_mjcf(p, keep_sites=("down",))
    assert full.names["rangefinder"] == {"height": 0, "_rangefinder1": 1, "again": 2}
    assert full.info["rangefinder"] == [dict(site="down", cutoff=0.0), dict(site="side", cutoff=0.5), dict(site="down", cutoff=3.0)]
    sim = BatchedSim(full, 2, outputs=("xpos", "xquat", "site_xpos", "site_xmat"))
    assert sim.n_rangefinder == 3 and sim.rangefinder_id("again") == 2
    with pytest.raises(KeyError):
        sim.rangefinder_id("t")
    with pytest.raises(ValueError, match="_rangefinder1"):      # its site was not kept
        BatchedSim(cut, 2, outputs=("xpos", "xquat", "site_xpos", "site_xmat")).rangefinder()
    with pytest.raises(ValueError, match="site_xpos"):          # the outputs a site ray needs, named
        BatchedSim(full, 2, outputs=("xpos", "xquat")).rangefinder()
    with pytest.raises(ValueError, match="xquat"):
        BatchedSim(full, 2, outputs=("xpos",)).ray(np.zeros((1, 3)), np.ones((1, 3)))

