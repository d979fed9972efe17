"""Ray casting (grx_sim_ray, BatchedSim.ray) against an fp64 reference: the reference, the ray sets and the acceptance rule both test files share
(tests/test_cpu_rays.py on the host build of csrc/grx_rays.h, tests/test_gpu_rays.py on the device).  Plain Python, numpy and scipy.

REFERENCE.  cast(): fp64 numpy over the oracle's geom_xpos / geom_xmat and the model tables, the closed forms of the definition in include/grx_capi.h (a ray o + t d, the
smallest t >= 0 on the surface of each eligible geom, the smallest of those, the smaller geom id on a tie, -1 for none); hull planes from
scipy.spatial.ConvexHull(...).equations on the hull's vertices.  check_reference() holds it to an independent route: each geom type's implicit inside-function f,
|f(hit)| < 1e-9, and no sample of [0, t_hit) on the other side of any eligible geom's surface from o.

RAY SETS.  Scene crowd-mixed of tests/contact_matrix_cases.py (a plane, the five primitives and both meshes, static and free, in each of 5 + 13 worlds), RAYS rays per world,
drawn from a generator seeded by the world: rays aimed at a point near the centre of every geom from 0.4 .. 1.5 m away (of any length, so t is not metres), rays that start
inside every solid, rays that leave the plane upwards, rays that miss everything, rays straight down, a zero and a NaN direction.  A launch of R rays takes the first R.

ACCEPTANCE.  Each ray is cast again by the reference alone under C.DRAWS jitter draws (origin moved by 1e-5 m, direction turned by 1e-5 rad).  A ray is COMPARED iff the hit
geom is the same in every draw (or it stays a miss) and dist moves by at most C.BOUND / 2: a condition on the reference from the reference alone.  Compared rays must agree
in geom exactly and in dist within C.BOUND * max(1, dist); every ray must be finite and -1 / -1 together.  At least 90 % of a world's rays must be compared."""
import numpy as np

import contact_matrix_cases as M
import engine_matrix_cases as C

RAYS = 130
SCENE = "crowd-mixed"
MIN_SHARE = 0.9
TYPE_NAMES = {0: "plane", 2: "sphere", 3: "capsule", 4: "ellipsoid", 5: "cylinder", 6: "box", 7: "mesh"}
_INF = np.inf


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the model's geoms
class Geoms:
    def __init__(self, model):
        tab = lambda k, w=None: (np.asarray(model.tables[k]).reshape(-1) if w is None else np.asarray(model.tables[k], dtype=np.float64).reshape(-1, w))
        self.type, self.body = tab("geom_type").astype(int), tab("geom_bodyid").astype(int)
        self.size, self.rbound = tab("geom_size", 3), np.asarray(model.tables["geom_rbound"], dtype=np.float64).reshape(-1)
        self.n = len(self.type)
        hadr, hnum, vert = tab("geom_hulladr").astype(int), tab("geom_hullnum").astype(int), tab("mesh_vert", 3)
        self.verts, self.planes = {}, {}
        for g in np.nonzero(self.type == 7)[0]:
            self.verts[g] = vert[hadr[g]:hadr[g] + hnum[g]]
            self.planes[g] = scipy_planes(self.verts[g])


def scipy_planes(vert):
    """[P, 4] (n, c) with n . x <= c inside: the facet equations of scipy's hull, the triangles of one face merged"""
    from scipy.spatial import ConvexHull

    eq = ConvexHull(np.asarray(vert, dtype=np.float64)).equations
    out = []
    for e in eq:
        p = np.r_[e[:3], -e[3]]
        if not any(np.abs(p - q).max() < 1e-9 for q in out):
            out.append(p)
    return np.array(out)


_GEOMS = {}


def geoms_of(model):
    if id(model) not in _GEOMS:
        _GEOMS[id(model)] = (model, Geoms(model))
    return _GEOMS[id(model)][1]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the reference: one geom against n rays in its own frame (p, d [n, 3]); t [n], inf = no hit
def _pick(cands):
    """smallest non-negative of the candidate columns (nan / negative = none)"""
    t = np.stack(cands, axis=1)
    t = np.where(np.isfinite(t) & (t >= 0), t, _INF)
    return t.min(axis=1)


def _roots(p, d, r):
    with np.errstate(all="ignore"):
        a, b, c = (d * d).sum(1), (d * p).sum(1), (p * p).sum(1) - r * r
        det = b * b - a * c
        sq = np.sqrt(np.where(det >= 0, det, np.nan))
        return (-b - sq) / a, (-b + sq) / a


def geom_hits(kind, size, planes, p, d):
    with np.errstate(all="ignore"):
        if kind == 0:
            t = -p[:, 2] / d[:, 2]
            ok = (d[:, 2] < 0) & (t >= 0)
            for k in (0, 1):
                if size[k] > 0:
                    ok &= np.abs(p[:, k] + t * d[:, k]) <= size[k]
            return np.where(ok, t, _INF)
        if kind == 2:
            return _pick(list(_roots(p, d, size[0])))
        if kind == 4:
            return _pick(list(_roots(p / size, d / size, 1.0)))
        if kind in (3, 5):
            r, h = size[0], size[1]
            cands = []
            for t in _roots(p[:, :2], d[:, :2], r):
                cands.append(np.where(np.abs(p[:, 2] + t * d[:, 2]) <= h, t, np.nan))
            for s in (1.0, -1.0):
                if kind == 3:
                    pe = p - [0.0, 0.0, s * h]
                    for t in _roots(pe, d, r):
                        cands.append(np.where(s * (pe[:, 2] + t * d[:, 2]) >= 0, t, np.nan))
                else:
                    t = (s * h - p[:, 2]) / d[:, 2]
                    x = p[:, :2] + t[:, None] * d[:, :2]
                    cands.append(np.where((x * x).sum(1) <= r * r, t, np.nan))
            return _pick(cands)
        if kind == 6:
            planes = np.array([[1.0, 0, 0, size[0]], [-1, 0, 0, size[0]], [0, 1, 0, size[1]], [0, -1, 0, size[1]], [0, 0, 1, size[2]], [0, 0, -1, size[2]]])
        nd, gap = d @ planes[:, :3].T, planes[:, 3] - p @ planes[:, :3].T      # [n, P]
        t = gap / nd
        enter = np.where(nd < 0, t, -_INF).max(axis=1)
        leave = np.where(nd > 0, t, _INF).min(axis=1)
        out = ((nd == 0) & (gap < 0)).any(axis=1)
        hit = np.where(enter >= 0, enter, leave)
        return np.where(~out & (enter <= leave) & (leave >= 0) & np.isfinite(hit), hit, _INF)


def cast(model, gxpos, gxmat, o, d, exclude_body=None, include_static=True, max_dist=0.0):
    """the reference: (dist [n], geom [n]) of the rays o, d [n, 3] against the geoms at gxpos [ngeom, 3], gxmat [ngeom, 9]"""
    G = geoms_of(model)
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    n = len(o)
    ex = np.full(n, -1) if exclude_body is None else np.broadcast_to(np.asarray(exclude_body), (n,))
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    best, who = np.full(n, _INF), np.full(n, -1)
    gxpos, gxmat = np.asarray(gxpos).reshape(-1, 3), np.asarray(gxmat).reshape(-1, 3, 3)
    for g in range(G.n):
        if G.body[g] == 0 and not include_static:
            continue
        R = gxmat[g]
        t = geom_hits(G.type[g], G.size[g], G.planes.get(g), (o - gxpos[g]) @ R, d @ R)
        t = np.where(valid & (ex != G.body[g]), t, _INF)
        better = t < best      # strict: the smaller id keeps a tie
        best, who = np.where(better, t, best), np.where(better, g, who)
    if max_dist > 0:
        best = np.where(best > max_dist, _INF, best)
    miss = ~np.isfinite(best)
    return np.where(miss, -1.0, best), np.where(miss, -1, who)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the independent route: implicit inside-functions
def inside_f(kind, size, planes, p):
    """f(p) <= 0 inside the solid, p [n, 3] in the geom's frame; a plane: the height above it"""
    if kind == 0:
        return p[:, 2]
    if kind == 2:
        return np.linalg.norm(p, axis=1) - size[0]
    if kind == 3:
        q = p.copy()
        q[:, 2] -= np.clip(q[:, 2], -size[1], size[1])
        return np.linalg.norm(q, axis=1) - size[0]
    if kind == 4:
        return np.linalg.norm(p / size, axis=1) - 1.0
    if kind == 5:
        return np.maximum(np.linalg.norm(p[:, :2], axis=1) - size[0], np.abs(p[:, 2]) - size[1])
    if kind == 6:
        return (np.abs(p) - size).max(axis=1)
    return (p @ planes[:, :3].T - planes[:, 3]).max(axis=1)


def check_reference(model, gxpos, gxmat, o, d, dist, geom, samples=400, reach=4.0):
    """every hit lies on its geom's surface, and the open segment before it crosses no eligible surface (a plane: not from above to below inside its bounds)"""
    G = geoms_of(model)
    gxpos, gxmat = np.asarray(gxpos).reshape(-1, 3), np.asarray(gxmat).reshape(-1, 3, 3)
    for r in range(len(o)):
        if not (np.isfinite(o[r]).all() and np.isfinite(d[r]).all() and np.any(d[r] != 0)):
            assert dist[r] == -1 and geom[r] == -1
            continue
        if geom[r] >= 0:
            g = geom[r]
            hit = ((o[r] + dist[r] * d[r] - gxpos[g]) @ gxmat[g])[None]
            assert abs(inside_f(G.type[g], G.size[g], G.planes.get(g), hit)[0]) < 1e-9, (r, g, "the hit is not on the surface")
        t_end = dist[r] if geom[r] >= 0 else reach / np.linalg.norm(d[r])
        ts = np.linspace(0.0, t_end, samples, endpoint=False)
        pts = o[r] + ts[:, None] * d[r]
        for g in range(G.n):
            loc = (pts - gxpos[g]) @ gxmat[g]
            f = inside_f(G.type[g], G.size[g], G.planes.get(g), loc)
            if G.type[g] == 0:
                inb = np.ones(len(loc), dtype=bool)
                for k in (0, 1):
                    if G.size[g][k] > 0:
                        inb &= np.abs(loc[:, k]) <= G.size[g][k]
                assert not ((f[:-1] > 1e-9) & (f[1:] < -1e-9) & inb[1:] & inb[:-1]).any(), (r, g, "the ray crosses the plane before its hit")
            else:
                s0 = f[0]
                assert not ((f * np.sign(s0) < -1e-9).any()) or abs(s0) < 1e-9, (r, g, "the ray crosses a surface before its hit")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the worlds of the scene and their rays
class World:
    """one world of crowd-mixed after forward(): the oracle's body and geom poses, its rays, the reference's answer and which rays are compared"""


_WORLDS = {}


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def _inner(G, g):
    """a length safely inside geom g about its centre"""
    if G.type[g] == 7:
        return 0.1 * G.rbound[g]
    s = G.size[g]
    return 0.2 * min(x for x in (s[:1] if G.type[g] == 2 else s[:2] if G.type[g] in (3, 5) else s) if x > 0)


def make_rays(model, gxpos, world, min_up=0.15):
    """min_up: the smallest upward component of the direction an aimed ray comes from, before normalisation.  A ray that meets a face at a shallow angle theta moves its dist by
    about (1e-5 + dist 1e-5 cos theta) / sin theta under the jitter, more than BOUND / 2 below some 25 degrees at 1.5 m: a scene with few geoms, where half of the aimed rays
    go to the floor, takes a larger min_up so that the reference alone keeps 90 % of the set"""
    G = geoms_of(model)
    rng = np.random.default_rng([0x7A9, C._name_seed(SCENE), world])
    o, d = np.zeros((RAYS, 3)), np.zeros((RAYS, 3))
    solids = [g for g in range(G.n) if G.type[g] != 0]
    for k in range(RAYS):
        if k < 90:      # aimed at geom k mod ngeom (the plane: at a point of it), from above or from the side
            g = k % G.n
            target = np.r_[rng.uniform(-0.4, 1.4, 2), 0.0] if G.type[g] == 0 else gxpos[g] + 1.5 * _inner(G, g) * _unit(rng)
            u = _unit(rng)
            u[2] = abs(u[2]) * (1.0 - min_up) + min_up
            o[k] = target + rng.uniform(0.4, 1.5) * u / np.linalg.norm(u)
            o[k, 2] = max(o[k, 2], 0.02)
            d[k] = (target - o[k]) * rng.uniform(0.5, 3.0)
        elif k < 108:   # starts inside a solid
            g = solids[(k - 90) % len(solids)]
            o[k], d[k] = gxpos[g] + _inner(G, g) * _unit(rng), _unit(rng) * rng.uniform(0.5, 2.0)
        elif k < 114:   # leaves the plane upwards from just above it: a one-sided plane is not hit from behind either (origin below, going up)
            o[k] = np.r_[rng.uniform(-1.5, -0.5, 2), 0.3 if k % 2 else -0.3]
            d[k] = np.r_[0.3 * rng.standard_normal(2), 1.0]
        elif k < 120:   # misses: above everything, level or rising
            o[k] = np.r_[rng.uniform(-0.5, 1.5, 2), rng.uniform(0.8, 1.2)]
            u = _unit(rng)
            d[k] = np.r_[u[:2], abs(u[2]) * 0.2]
        elif k < 128:   # straight down or nearly, somewhere over the scene
            o[k] = np.r_[rng.uniform(-0.3, 1.3, 2), rng.uniform(0.5, 1.0)]
            d[k] = np.r_[0.05 * rng.standard_normal(2), -1.0] * rng.uniform(0.5, 2.0)
        elif k == 128:
            o[k], d[k] = [0.3, 0.3, 0.5], 0.0
        else:
            o[k], d[k] = [0.3, 0.3, 0.5], [np.nan, 0.0, -1.0]
    perm = np.r_[rng.permutation(128), 128, 129]      # a launch of the first R rays holds every kind
    return C.f32(o[perm]), C.f32(d[perm])


def jitter(o, d, rng):
    """one draw: every origin moved by 1e-5 m in a random direction, every direction turned by 1e-5 rad about a random axis"""
    n = len(o)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(d, rng.standard_normal((n, 3)))
    with np.errstate(all="ignore"):
        v = np.where(np.isfinite(v).all(1, keepdims=True) & (np.linalg.norm(v, axis=1, keepdims=True) > 0), v / np.linalg.norm(v, axis=1, keepdims=True), 0.0)
        dj = np.cos(1e-5) * d + np.sin(1e-5) * np.linalg.norm(d, axis=1, keepdims=True) * v
    return o + 1e-5 * u, np.where(np.isfinite(d), dj, d)


def compared_mask(model, gxpos, gxmat, o, d, dist, geom, seed, **kw):
    rng = np.random.default_rng([0x6A17, C._name_seed(SCENE)] + list(seed))
    ok = np.ones(len(o), dtype=bool)
    for _ in range(C.DRAWS):
        oj, dj = jitter(o, d, rng)
        dist_j, geom_j = cast(model, gxpos, gxmat, oj, dj, **kw)
        ok &= (geom_j == geom) & (np.abs(dist_j - dist) <= C.BOUND / 2)
    return ok


def world(variant, i):
    """world i of variant `variant` (0: the launch of 5 worlds, 1: of 13) of the scene, built once: read only"""
    key = (variant, i)
    if key not in _WORLDS:
        var = M.group(SCENE).variants[variant]
        sim = M._sim(var)
        sim.reset_data()
        sim.qpos[:], sim.qvel[:], sim.qacc_warmstart[:] = var.q0[i], var.v0[i], 0.0
        sim.forward()
        w = World()
        w.model, w.index = var.model, var.idx[i]
        w.xpos, w.xquat = sim.xpos.reshape(-1, 3).copy(), sim.xquat.reshape(-1, 4).copy()
        w.gxpos, w.gxmat = sim.geom_xpos.reshape(-1, 3).copy(), sim.geom_xmat.reshape(-1, 9).copy()
        w.o, w.d = make_rays(w.model, w.gxpos, w.index)
        w.dist, w.geom = cast(w.model, w.gxpos, w.gxmat, w.o, w.d)
        w.compared = compared_mask(w.model, w.gxpos, w.gxmat, w.o, w.d, w.dist, w.geom, (w.index,))
        _WORLDS[key] = w
    return _WORLDS[key]


def n_worlds(variant):
    return len(M.group(SCENE).variants[variant].idx)


def accept(tag, model, dist, geom, want_dist, want_geom, compared, worst):
    """the acceptance rule for one world's rays; worst: dict geom type name -> worst error of the compared rays, updated in place.  Prints before it asserts."""
    dist, geom = np.asarray(dist, dtype=np.float64), np.asarray(geom)
    assert np.isfinite(dist).all(), (tag, "non-finite dist (a NaN is an element the launch did not write)")
    assert ((dist == -1.0) == (geom == -1)).all() and (geom >= -1).all() and ((dist >= 0) | (dist == -1.0)).all(), (tag, "dist and geom disagree about a miss")
    G = geoms_of(model)
    err = np.abs(dist - want_dist) / np.maximum(1.0, np.abs(want_dist))
    bad = [(int(r), int(geom[r]), int(want_geom[r]), float(dist[r]), float(want_dist[r])) for r in np.nonzero(compared)[0] if geom[r] != want_geom[r] or not err[r] <= C.BOUND]
    for r in np.nonzero(compared & (want_geom >= 0) & (geom == want_geom))[0]:
        name = TYPE_NAMES[int(G.type[want_geom[r]])]
        worst[name] = max(worst.get(name, 0.0), float(err[r]))
    print(f"{tag}: compared {int(compared.sum())} / {len(compared)}, worst error {float(err[compared].max()) if compared.any() else 0.0:.2e}")
    assert not bad, (tag, "(ray, geom, reference geom, dist, reference dist) of the compared rays that disagree", bad)


def record(kind, worst):
    """with GRX_RECORD_RAY_ERRORS set: the worst error of the compared rays per geom type, as measured by this run, into tests/golden/ray_errors.json under `kind`
    ("host": the routines compiled for the CPU, "mi355x": the kernel)"""
    import json
    import os

    if not os.environ.get("GRX_RECORD_RAY_ERRORS"):
        return
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_errors.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["bound"] = "|dist - reference| <= %g * max(1, dist) on the compared rays of crowd-mixed, geom equal" % C.BOUND
    doc[kind] = {k: float("%.3g" % v) for k, v in sorted(worst.items())}
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
