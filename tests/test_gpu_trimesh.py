"""Mesh triangles on the device (mesh="triangles": grx_sim_ray_tri, grx_sim_render_tri) against tests/trimesh_cases.py under the rule of tests/ray_cases.py; outputs start as NaN / a sentinel."""
import numpy as np
import pytest

import camera_cases as K
import engine_matrix_cases as C
import ray_cases as R
import trimesh_cases as T
from test_gpu_camera import FOVY, _images
from test_gpu_rays import _filled, _sim

pytestmark = pytest.mark.gpu


def _scene(name, spare=True):      # the scene's three worlds after forward(): the simulation and the body poses the device holds, in fp64
    sim = _sim(T.model(name, spare), T.N, T.Q0[:, :14 if spare else 7], np.zeros((T.N, 12 if spare else 6)))
    sim.forward()
    return sim, sim.xpos.cpu().numpy().astype(np.float64), sim.xquat.cpu().numpy().astype(np.float64)


def _rule_model(name, made={}):
    """the model as ray_cases.accept reads it, once per mesh: it looks at geom types only, but derives hull planes for every mesh geom first: seconds for the fine torus's
    1000-vertex hull, a failure for `bare`, which has none.  Both mesh geoms name eight spread vertices of `mesh`'s hull here"""
    if name not in made:
        m = T.model(name).copy()
        g, t = m.names["geom"], m.tables
        adr, num = int(t["geom_hulladr"][g["mesh"]]), int(t["geom_hullnum"][g["mesh"]])
        t["mesh_vert"] = np.concatenate([np.asarray(t["mesh_vert"]).reshape(-1, 3), np.asarray(t["mesh_vert"]).reshape(-1, 3)[adr + np.linspace(0, num - 1, 8).astype(int)]])
        for k in ("mesh", "bare"):
            t["geom_hulladr"][g[k]], t["geom_hullnum"][g[k]] = len(t["mesh_vert"]) - 8, 8
        made[name] = m
    return made[name]


@pytest.mark.parametrize("name", T.MESHES)
def test_rays_see_the_triangles(name):
    """257 rays per world (a block and one ray) against one or two leaves, a hierarchy of several levels and one of 2047 nodes; the rays through the notch / the hole hit what
    lies behind, where the hull path -- on the scene without `bare`, which it refuses -- reports the hull"""
    import torch

    sim, xpos, xquat = _scene(name)
    worlds = [T.world(name, i, xpos[i], xquat[i]) for i in range(T.N)]
    o, d = (torch.tensor(np.stack([getattr(w, k) for w in worlds]), dtype=torch.float32, device=sim.device) for k in ("o", "d"))
    dist, geom = (x.cpu().numpy() for x in sim.ray(o, d, mesh="triangles", out=_filled(sim, T.RAYS)))
    with pytest.raises(ValueError, match="no full hull"):
        sim.ray(o, d)
    sim.close()
    hull, _, _ = _scene(name, spare=False)
    hull_geom = hull.ray(o, d)[1].cpu().numpy()
    hull.close()
    mesh_id = T.model(name).names["geom"]["mesh"]
    for i, w in enumerate(worlds):
        R.accept(("mi355x", name, i), _rule_model(name), dist[i], geom[i], w.dist, w.geom, w.compared, {})
        assert w.compared.mean() >= R.MIN_SHARE, (i, w.compared.mean())
        assert (hull_geom[i][w.through] == mesh_id).all() and (geom[i][w.through] != mesh_id).all(), "a ray through the gap: the hull stops it, the triangles do not"
    assert sum(int(w.through.sum()) for w in worlds) >= 20


@pytest.mark.parametrize("name, h, w", [("torus16", 17, 33), ("torus16", 64, 64), ("torus64", 17, 33), ("torus64", 64, 64)])
def test_cameras_see_the_triangles(name, h, w):
    """ragged edge tiles both ways and an image of 64 tiles; a hierarchy inside the kernel's LDS window (127 nodes) and one outside (2047); two steep, near cameras (a far or
    shallow floor pixel does not survive the jitter).  Unbinned: the same bits.  A masked-out world reads -1."""
    import torch

    sim, xpos, xquat = _scene(name)
    m, tri = T.model(name), T.file_triangles(name)
    geoms = [T.poses(m, xpos[i], xquat[i]) for i in range(T.N)]
    at = np.array([gx[m.names["geom"]["mesh"]] for gx, _ in geoms])
    pos = C.f32(np.stack([at + [0.15, -0.2, 0.9], at + [0.25, 0.15, 0.75]], axis=1))
    mat = C.f32(np.array([[K.look_at(pos[i, j], at[i]) for j in (0, 1)] for i in range(T.N)]))
    depth, seg = _images(sim.render_pose, sim, 2, h, w, pos, mat, FOVY, mesh="triangles")
    plain = _images(sim.render_pose, sim, 2, h, w, pos, mat, FOVY, mesh="triangles", binning=False)
    assert np.array_equal(plain[0], depth) and np.array_equal(plain[1], seg)
    fresh = sim.render_pose(pos, mat, FOVY, h, w, segmentation=True, mesh="triangles", mask=torch.tensor([1, 0, 1], dtype=torch.uint8, device=sim.device))
    assert (fresh[0][1] == -1).all() and (fresh[1][1] == -1).all() and np.array_equal(fresh[0][[0, 2]].cpu().numpy(), depth[[0, 2]])
    sim.close()
    seen = set()
    for i, (gx, gm) in enumerate(geoms):
        for j in (0, 1):
            o, d = K.fan(pos[i, j], mat[i, j], FOVY, h, w)
            want_depth, want_seg, pairs = T.cast(m, tri, gx, gm, o, d)
            compared = T.compared(m, tri, gx, gm, o, d, want_depth, want_seg, pairs, (i, j, h))
            R.accept(("mi355x", name, h, w, i, "AB"[j]), _rule_model(name), depth[i, j].ravel(), seg[i, j].ravel(), want_depth, want_seg, compared, {})
            assert compared.mean() >= R.MIN_SHARE, (i, j, compared.mean())
            seen |= set(want_seg[compared].tolist())
    assert seen >= {0, m.names["geom"]["mesh"]}, "the images show the floor and the torus"


def test_a_model_without_a_mesh_gives_the_same_bits():
    import torch

    model = C.compile_xml(K.XML)
    sim = _sim(model, 3, np.array([[0.0], [0.7], [-1.1]]), np.zeros((3, 1)))
    sim.forward()
    rng = np.random.default_rng(5)
    o = torch.tensor(rng.uniform([-1, -1, 1.5], [2, 2, 2.5], (3, 130, 3)), dtype=torch.float32, device=sim.device)
    d = torch.tensor(rng.standard_normal((3, 130, 3)) * [0.5, 0.5, 0.2] - [0, 0, 1], dtype=torch.float32, device=sim.device)
    a, b = sim.ray(o, d, out=_filled(sim, 130)), sim.ray(o, d, mesh="triangles", out=_filled(sim, 130))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (a[1] >= 0).any() and int(a[1].max()) > 0
    a, b = _images(sim.render, sim, 1, 17, 33, "overview"), _images(sim.render, sim, 1, 17, 33, "overview", mesh="triangles")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(np.unique(a[1])) >= 3
    sim.close()
