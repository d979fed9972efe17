"""Rays and cameras that see mesh TRIANGLES (mesh="triangles"): the scene, the fp64 reference and the ray sets of tests/test_cpu_trimesh.py and tests/test_gpu_trimesh.py.
SCENE: a floor, a box, a sphere, the mesh of a fixture (tests/golden/trimesh_*.stl) with a scale on a free body, its geom turned, and -- `spare` -- the same mesh on a second
free body that can only meet the floor, so it keeps no hull: the geom the hull path refuses.  Three worlds with different free-joint poses.
REFERENCE: cast(), fp64 Moeller-Trumbore over the file's triangles in the hull vertices' frame, ray_cases.geom_hits for the primitives.  No hierarchy: near() only drops the
(ray, triangle) pairs whose triangle lies farther from the ray's LINE than its own radius plus 2 mm per metre, two hundred times what the jitter moves a ray.
ACCEPTANCE: ray_cases.accept on the rays the reference reproduces under ray_cases.jitter (compared())."""
import os
import types

import numpy as np

import engine_matrix_cases as C
import ray_cases as R
from gymnasium_robotics_amd.mjcf import mathutil as mu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MESHES = {"bracket": "trimesh_bracket.stl", "torus16": "trimesh_torus_16x8.stl", "torus64": "trimesh_torus_64x32.stl"}
SCALE = np.array([0.3, 0.28, 0.35])
N, RAYS = 3, 257
Q0 = C.f32([[0.1, 0.0, 0.8, 0.95, 0.2, 0.1, 0.2, -0.7, -0.5, 0.6, 0.9, 0.3, 0.0, -0.3], [0.0, 0.2, 0.9, 0.8, -0.3, 0.4, 0.1, -0.6, -0.7, 0.5, 1.0, 0.0, 0.0, 0.0],
            [-0.1, 0.1, 0.7, 0.7, 0.1, -0.2, 0.6, -0.8, -0.4, 0.7, 0.6, 0.1, 0.5, 0.2]])      # qpos: the two free bodies (the engine normalises the quaternions)
_MODELS = {}


def model(name, spare=True):
    if (name, spare) not in _MODELS:
        _MODELS[name, spare] = C.compile_xml(f"""<mujoco><compiler meshdir="{GOLDEN}"/><asset><mesh name="m" file="{MESHES[name]}" scale="{SCALE[0]} {SCALE[1]} {SCALE[2]}"/></asset><worldbody>
  <geom name="floor" type="plane" size="3 3 0.1" contype="3" conaffinity="3"/>
  <geom name="post" type="box" size="0.1 0.15 0.3" pos="0.8 0.3 0.3"/><geom name="ball" type="sphere" size="0.15" pos="-0.5 0.6 0.4"/>
  <body name="part" pos="0 0 0.8"><freejoint/><geom name="mesh" type="mesh" mesh="m" quat="0.9 0.1 0.3 0.2" mass="1"/></body>
  {'<body name="spare" pos="-0.7 -0.5 0.6"><freejoint/><geom name="bare" type="mesh" mesh="m" quat="0.8 -0.2 0.1 0.4" mass="1" contype="2" conaffinity="2"/></body>' if spare else ''}
</worldbody></mujoco>""")
    return _MODELS[name, spare]


def file_triangles(name):
    """[T, 3, 3] fp64: the fixture's triangles, scaled, in the compiled geom frame -- found from the hull vertices the model's blob holds for geom `mesh`, not from the compiler"""
    from scipy.spatial import ConvexHull

    raw = np.fromfile(os.path.join(GOLDEN, MESHES[name]), dtype=np.uint8)[84:].reshape(-1, 50)[:, 12:48].copy().view("<f4").reshape(-1, 3, 3).astype(np.float64) * SCALE
    m, v = model(name), np.unique(raw.reshape(-1, 3), axis=0)
    g = m.names["geom"]["mesh"]
    adr, num = int(m.tables["geom_hulladr"][g]), int(m.tables["geom_hullnum"][g])
    return raw - (v[ConvexHull(v).vertices].mean(axis=0) - np.asarray(m.tables["mesh_vert"], dtype=np.float64).reshape(-1, 3)[adr:adr + num].mean(axis=0))


def poses(m, xpos, xquat):
    """geom_xpos [ngeom, 3], geom_xmat [ngeom, 3, 3] in fp64 from the body poses of one world"""
    t = m.tables
    body, gp, gq = np.asarray(t["geom_bodyid"]).reshape(-1), np.asarray(t["geom_pos"], dtype=np.float64).reshape(-1, 3), np.asarray(t["geom_quat"], dtype=np.float64).reshape(-1, 4)
    xpos, xquat = np.asarray(xpos, dtype=np.float64).reshape(-1, 3), np.asarray(xquat, dtype=np.float64).reshape(-1, 4)
    return (np.array([xpos[b] + mu.quat2mat(xquat[b]) @ p for b, p in zip(body, gp)]), np.array([mu.quat2mat(xquat[b]) @ mu.quat2mat(q / np.linalg.norm(q)) for b, q in zip(body, gq)]))


def near(p, d, tri):
    """(ray, triangle) pairs that can meet (module docstring); p, d [n, 3] in the mesh's frame.  Rays whose line passes the whole mesh's sphere by are dropped first"""
    miss = lambda c, rad, w, u: np.linalg.norm(np.cross(w, u), axis=-1) > rad + 2e-3 * (1.0 + np.linalg.norm(w, axis=-1))
    u, c0, c = d / np.linalg.norm(d, axis=1, keepdims=True), tri.reshape(-1, 3).mean(axis=0), tri.mean(axis=1)
    rays = np.nonzero(~miss(c0, np.linalg.norm(tri.reshape(-1, 3) - c0, axis=1).max(), c0 - p, u))[0]
    rad, out = np.linalg.norm(tri - c[:, None], axis=2).max(axis=1), [(np.zeros(0, int), np.zeros(0, int))]
    for s in range(0, len(rays), 256):
        r, k = np.nonzero(~miss(c, rad[None], c[None] - p[rays[s:s + 256], None], u[rays[s:s + 256], None]))
        out.append((rays[s:s + 256][r], k))
    return np.concatenate([x[0] for x in out]), np.concatenate([x[1] for x in out])


def mesh_hits(p, d, tri, pairs):
    """fp64 Moeller-Trumbore, two-sided, on the pairs; the smallest t >= 0 per ray, inf for none"""
    r, k = pairs
    v0, e1, e2 = tri[k, 0], tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0]
    with np.errstate(all="ignore"):
        pv, tv = np.cross(d[r], e2), p[r] - v0
        det, qv = (e1 * pv).sum(1), np.cross(tv, e1)
        u, v, t = (tv * pv).sum(1) / det, (d[r] * qv).sum(1) / det, (e2 * qv).sum(1) / det
    best = np.full(len(p), np.inf)
    np.minimum.at(best, r, np.where((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0), t, np.inf))
    return best


def cast(m, tri, gx, gm, o, d, pairs=None, mesh="triangles"):
    """(dist [n], geom [n], pairs): the nearest hit over the model's geoms, the smaller id on a tie; pairs: near() per mesh geom, reused for the jittered casts of the same rays"""
    kind, size = np.asarray(m.tables["geom_type"]).reshape(-1), np.asarray(m.tables["geom_size"], dtype=np.float64).reshape(-1, 3)
    best, who, pairs = np.full(len(o), np.inf), np.full(len(o), -1), dict(pairs or {})
    for g in range(len(kind)):
        p, dl = (o - gx[g]) @ gm[g], d @ gm[g]
        if kind[g] == 7 and mesh == "triangles":
            if g not in pairs:
                pairs[g] = near(p, dl, tri)
            t = mesh_hits(p, dl, tri, pairs[g])
        else:
            t = R.geom_hits(kind[g], size[g], R.scipy_planes(tri.reshape(-1, 3)) if kind[g] == 7 else None, p, dl)
        better = t < best
        best, who = np.where(better, t, best), np.where(better, g, who)
    return np.where(np.isfinite(best), best, -1.0), np.where(np.isfinite(best), who, -1), pairs


def compared(m, tri, gx, gm, o, d, dist, geom, pairs, seed):
    """ray_cases.compared_mask over this reference: the rays whose hit the reference reproduces under every jitter draw"""
    rng, ok = np.random.default_rng([0x7B1] + list(seed)), np.ones(len(o), dtype=bool)
    for _ in range(C.DRAWS):
        dist_j, geom_j, _ = cast(m, tri, gx, gm, *R.jitter(o, d, rng), pairs)
        ok &= (geom_j == geom) & (np.abs(dist_j - dist) <= C.BOUND / 2)
    return ok


def make_rays(name, tri, gx, gm, world, n_hole=24):
    """RAYS fp32 rays of one world: n_hole through the notch / hole of geom `mesh` along its axis and, filling the half aimed at the mesh from outside, rays onto a point of a
    triangle within 35 degrees of its normal; a quarter that start inside the mesh's bounds; the rest aimed at the other geoms"""
    rng, g = np.random.default_rng([0x7B0, world]), model(name).names["geom"]["mesh"]
    unit = lambda k: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.standard_normal((k, 3)))
    shift = (tri.reshape(-1, 3).min(axis=0) + tri.reshape(-1, 3).max(axis=0)) / 2 - ([0.3, 0.3, 0.15] * SCALE if name == "bracket" else 0.0)      # file origin in the geom frame
    rho, phi = 0.2 * np.sqrt(rng.uniform(0, 1, n_hole)), rng.uniform(0, 2 * np.pi, n_hole)      # file coordinates: the bracket's notch, the torus's hole (outside the mesh, inside its hull)
    gap = np.c_[rng.uniform(0.25, 0.33, (n_hole, 2)) if name == "bracket" else np.c_[rho * np.cos(phi), rho * np.sin(phi)], np.zeros(n_hole)]
    po = gap * SCALE + shift + [0, 0, 0.5]
    o_l, d_l = [po], [np.c_[0.015 * rng.standard_normal((n_hole, 2)), -np.ones(n_hole)]]
    k = rng.integers(0, len(tri), RAYS // 2 - n_hole)
    w = rng.dirichlet([1, 1, 1], len(k))
    nrm = np.cross(tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0])
    out = nrm / np.linalg.norm(nrm, axis=1, keepdims=True) + 0.6 * unit(len(k)) * rng.uniform(0, 1, (len(k), 1))
    o_l.append((w[:, :, None] * tri[k]).sum(axis=1) + rng.uniform(0.3, 0.6, (len(k), 1)) * out)
    d_l.append(-out * rng.uniform(0.5, 2.0, (len(k), 1)))
    lo, hi = tri.reshape(-1, 3).min(axis=0), tri.reshape(-1, 3).max(axis=0)
    o_l.append(rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), (RAYS // 4, 3)))
    d_l.append(unit(RAYS // 4))
    o, d = np.concatenate(o_l) @ gm[g].T + gx[g], np.concatenate(d_l) @ gm[g].T
    rest = RAYS - len(o)      # from above, steeply, at the floor and at the other geoms' centres
    target = np.where(np.arange(rest)[:, None] % 4 == 0, np.c_[rng.uniform(-1.2, 1.2, (rest, 2)), np.zeros(rest)], gx[1 + np.arange(rest) % (len(gx) - 1)] + 0.03 * unit(rest))
    up = unit(rest) * [0.5, 0.5, 1.0]
    up[:, 2] = np.abs(up[:, 2]) + 0.5
    o2 = target + rng.uniform(0.4, 1.0, (rest, 1)) * up
    return C.f32(np.concatenate([o, o2])), C.f32(np.concatenate([d, (target - o2) * rng.uniform(0.5, 2.0, (rest, 1))]))


def world(name, i, xpos=None, xquat=None):
    """world i of mesh `name`'s scene (body poses: qpos Q0[i]'s by default): geom poses, rays, the reference's answer, the compared rays, and those that pass the notch / hole"""
    w, m, tri = types.SimpleNamespace(), model(name), file_triangles(name)
    if xpos is None:      # what forward() computes for bodies that hang on the world
        q = Q0[i]
        xpos, xquat = np.array([[0, 0, 0], q[0:3], q[7:10]]), np.array([[1, 0, 0, 0], q[3:7] / np.linalg.norm(q[3:7]), q[10:14] / np.linalg.norm(q[10:14])])
    w.gx, w.gm = poses(m, xpos, xquat)
    w.o, w.d = make_rays(name, tri, w.gx, w.gm, i)
    w.dist, w.geom, pairs = cast(m, tri, w.gx, w.gm, w.o, w.d)
    w.compared = compared(m, tri, w.gx, w.gm, w.o, w.d, w.dist, w.geom, pairs, (i,))
    w.through = w.compared & (np.arange(RAYS) < 24) & (w.geom != m.names["geom"]["mesh"]) & (w.geom >= 0)
    return w
