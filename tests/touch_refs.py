"""An independent fp64 reference for touch sensors (mjSENS_TOUCH), written from the definition and not from the device's formulas.  Plain numpy.

DEFINITION.  A touch sensor is a zone (a sphere, box or cylinder site) on a body.  Its reading is the sum of the normal forces of the contacts that
  - involve the zone's body (it is one of the contact's two bodies),
  - have constraint rows,
  - carry a normal force > 0,
  - and whose half line {p + t d, t >= 0} meets the SOLID zone: p is the contact point, d the contact normal, negated when the zone's body is the contact's second
    body.  An origin inside the zone meets it.

DECISION.  "Meets the solid zone" is decided by interval clipping in the zone's frame, never by picking roots:
  box ....... the three slab intervals intersected with [0, inf);
  sphere .... the origin is inside, or the closest point of the line lies ahead (p . d < 0) and within r of the centre;
  cylinder .. the infinite cylinder's interval, the z-slab's interval and [0, inf) intersected.

MARGIN.  Per (zone, contact) pair, how far the ray has to be moved (translated, in metres) before the decision can flip: the zones are convex, so their signed distance
functions are convex and s(t) = sdf(p + t d) has one minimum over t >= 0, found by golden section.  A hit with min s = -m keeps a point m deep inside under any
translation shorter than m; a miss with min s = +m stays outside.  The sign of min s is a second, independent decision: the two must agree wherever m > 1e-9, which
touch_reference asserts.  The margin says nothing about turning the ray; the cases are chosen so that a turn of the size the engines differ by moves the ray far less."""
import numpy as np

SPHERE, CYLINDER, BOX = 2, 5, 6
TYPE_NAMES = {SPHERE: "sphere", CYLINDER: "cylinder", BOX: "box"}
_INF = np.inf


def quat_to_mat(q):
    """[..., 3, 3] rotation matrices of unit quaternions [..., 4] (w, x, y, z): the columns are the frame's axes"""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = (q[..., k] for k in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def zone_world_poses(body, pos, quat, xpos, xquat):
    """(centre [nz, 3], R [nz, 3, 3]) of zones given in their bodies' frames (pos, quat) on bodies at xpos / xquat"""
    body = np.asarray(body, dtype=int)
    Rb = quat_to_mat(np.asarray(xquat, dtype=np.float64).reshape(-1, 4)[body])
    centre = np.asarray(xpos, dtype=np.float64).reshape(-1, 3)[body] + np.einsum("zij,zj->zi", Rb, np.asarray(pos, dtype=np.float64).reshape(-1, 3))
    return centre, Rb @ quat_to_mat(np.asarray(quat, dtype=np.float64).reshape(-1, 4))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# "the half line meets the solid": interval clipping.  p, d [n, 3] in the zone's frame, d not zero
def _clip_slab(lo, hi, p, d, h):
    """[lo, hi] intersected with {t : |p + t d| <= h} for one coordinate; an empty interval is lo > hi"""
    with np.errstate(all="ignore"):
        t1, t2 = (-h - p) / d, (h - p) / d
    par = d == 0
    a, b = np.where(par, np.where(np.abs(p) <= h, -_INF, _INF), np.minimum(t1, t2)), np.where(par, np.where(np.abs(p) <= h, _INF, -_INF), np.maximum(t1, t2))
    return np.maximum(lo, a), np.minimum(hi, b)


def _clip_disc(lo, hi, p, d, r):
    """[lo, hi] intersected with {t : |p + t d| <= r}, p and d [n, k]"""
    a, b, c = (d * d).sum(1), (p * d).sum(1), (p * p).sum(1) - r * r
    with np.errstate(all="ignore"):
        det = b * b - a * c
        sq = np.sqrt(np.maximum(det, 0.0))
        t1, t2 = (-b - sq) / a, (-b + sq) / a
    par = a == 0      # the ray runs along the axis: inside for every t or for none
    t1 = np.where(par, np.where(c <= 0, -_INF, _INF), np.where(det >= 0, t1, _INF))
    t2 = np.where(par, np.where(c <= 0, _INF, -_INF), np.where(det >= 0, t2, -_INF))
    return np.maximum(lo, t1), np.minimum(hi, t2)


def meets(kind, size, p, d):
    """[n] bool: the half line from p along d meets the solid zone of the given type and size (its own frame)"""
    p, d = np.asarray(p, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if kind == SPHERE:
        r = size[0]
        inside = (p * p).sum(1) <= r * r
        ahead = (p * d).sum(1) < 0
        with np.errstate(all="ignore"):
            foot = p - ((p * d).sum(1) / (d * d).sum(1))[:, None] * d      # the line's closest point to the centre
        return inside | (ahead & ((foot * foot).sum(1) <= r * r))
    lo, hi = np.zeros(n), np.full(n, _INF)
    if kind == BOX:
        for k in range(3):
            lo, hi = _clip_slab(lo, hi, p[:, k], d[:, k], size[k])
    elif kind == CYLINDER:
        lo, hi = _clip_disc(lo, hi, p[:, :2], d[:, :2], size[0])
        lo, hi = _clip_slab(lo, hi, p[:, 2], d[:, 2], size[1])
    else:
        raise ValueError(f"zone type {kind}")
    return lo <= hi


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the margin: signed distance functions of the three convex solids (exact outside and inside), minimised over the half line
def sdf(kind, size, x):
    x = np.asarray(x, dtype=np.float64)
    if kind == SPHERE:
        return np.linalg.norm(x, axis=-1) - size[0]
    if kind == BOX:
        q = np.abs(x) - np.asarray(size, dtype=np.float64)[:3]
    else:
        q = np.stack([np.linalg.norm(x[..., :2], axis=-1) - size[0], np.abs(x[..., 2]) - size[1]], axis=-1)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)


def inside(kind, size, x):
    """point-in-solid, from the solids' defining inequalities (the sampling check's route: no distances)"""
    x = np.asarray(x, dtype=np.float64)
    if kind == SPHERE:
        return (x * x).sum(-1) <= size[0] ** 2
    if kind == BOX:
        return (np.abs(x) <= np.asarray(size, dtype=np.float64)[:3]).all(-1)
    return ((x[..., :2] ** 2).sum(-1) <= size[0] ** 2) & (np.abs(x[..., 2]) <= size[1])


_GOLD = (np.sqrt(5.0) - 1.0) / 2.0


def min_sdf(kind, size, p, d):
    """[n]: min over t >= 0 of sdf(p + t d), d of any non-zero length; s(t) is convex, so golden section on [0, T] with T past the zone finds it to ~1e-12 m"""
    p, d = np.asarray(p, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    a, b = np.zeros(len(p)), np.linalg.norm(p, axis=1) + 2.0 * float(np.linalg.norm(np.asarray(size, dtype=np.float64)[:3])) + 1e-3
    f = lambda t: sdf(kind, size, p + t[:, None] * u)
    x1, x2 = b - _GOLD * (b - a), a + _GOLD * (b - a)
    f1, f2 = f(x1), f(x2)
    for _ in range(90):
        left = f1 <= f2
        b, a = np.where(left, x2, b), np.where(left, a, x1)
        x1n, x2n = b - _GOLD * (b - a), a + _GOLD * (b - a)
        f1, f2, x1, x2 = np.where(left, f(x1n), f2), np.where(left, f1, f(x2n)), x1n, x2n
    return np.minimum(np.minimum(f(a), f(b)), sdf(kind, size, p))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def touch_reference(zones, contacts):
    """zones: dict(body [nz], type [nz], pos [nz, 3] world centre, mat [nz, 3, 3] world axes as columns, size [nz, 3]).
    contacts: dict(body [nc, 2] the two bodies, pos [nc, 3], normal [nc, 3], force [nc] normal force, rows [nc] bool: has constraint rows).
    Returns (reading [nz], info) with info = dict(hit [nz, nc] the ray meets the zone, involved [nz, nc] the zone's body is one of the two,
    counted [nz, nc] the contact adds its force, margin [nz, nc] metres; inf where the zone's body is not involved)."""
    body, kind = np.asarray(zones["body"], dtype=int).reshape(-1), np.asarray(zones["type"], dtype=int).reshape(-1)
    zpos, zmat = np.asarray(zones["pos"], dtype=np.float64).reshape(-1, 3), np.asarray(zones["mat"], dtype=np.float64).reshape(-1, 3, 3)
    size = np.asarray(zones["size"], dtype=np.float64).reshape(-1, 3)
    cb = np.asarray(contacts["body"], dtype=int).reshape(-1, 2)
    cpos, cn = np.asarray(contacts["pos"], dtype=np.float64).reshape(-1, 3), np.asarray(contacts["normal"], dtype=np.float64).reshape(-1, 3)
    force, rows = np.asarray(contacts["force"], dtype=np.float64).reshape(-1), np.asarray(contacts["rows"], dtype=bool).reshape(-1)
    nz, nc = len(body), len(cb)
    hit, involved = np.zeros((nz, nc), dtype=bool), np.zeros((nz, nc), dtype=bool)
    margin = np.full((nz, nc), _INF)
    for z in range(nz):
        first, second = cb[:, 0] == body[z], cb[:, 1] == body[z]
        sel = np.nonzero(first | second)[0]
        involved[z, sel] = True
        if not len(sel):
            continue
        d = np.where(second[sel, None], -cn[sel], cn[sel])      # a self contact does not exist: first and second never hold together
        p = (cpos[sel] - zpos[z]) @ zmat[z]      # world -> zone frame: R' (x - c)
        d = d @ zmat[z]
        hit[z, sel] = meets(kind[z], size[z], p, d)
        s = min_sdf(kind[z], size[z], p, d)
        margin[z, sel] = np.abs(s)
        clash = (np.abs(s) > 1e-9) & ((s < 0) != hit[z, sel])
        assert not clash.any(), ("interval clipping and the distance minimum disagree", z, sel[clash], s[clash])
    counted = hit & involved & rows[None, :] & (force[None, :] > 0)
    reading = np.where(counted, force[None, :], 0.0).sum(axis=1)
    return reading, dict(hit=hit, involved=involved, counted=counted, margin=margin)
