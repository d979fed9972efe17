"""Generated scenes for the generic engine (GrxEngine<GrxShapeAny>, grx_point_step with agent = 1) against the fp64 oracle: deterministic case tables and the
helpers both test files share (tests/test_cpu_engine_matrix.py on the lane emulator, tests/test_gpu_engine_matrix.py on the device).  Plain Python and numpy.

A. pair groups ... geom A on a free joint against geom B (a plane, a static geom, or a geom on its own free joint) at random relative poses, pressed in by
                   0.3 .. 3 mm, plus hand-placed poses next to the degenerate ones (parallel capsules, a sphere centre inside a box, stacked boxes ...)
B. tree groups ... contact-free random trees of hinge / slide joints, half of them on a free root, with limits, friction loss, springs, actuators; Euler and RK4
                   (no ball joints: neither the engine nor the oracle has one, and the compiler refuses them)
C. solve groups .. hinge / slide trees of an exact nv (every route of grx_sym_solve_full), and robots followed by a free body (the block-diagonal routes)
D. row groups .... welds, joint equalities, fixed-tendon limits, affine and clamped actuators, two actuators on one joint, impratio and noslip: one model each, and
                   two of nv = 20 that hold all five row kinds in one world (Euler and RK4)

condim and margin / gap are properties of the MODEL in MJCF, so a pair group is compiled in up to eight VARIANTS (condim 1 / 3 / 4 / 6, with and without
margin="0.004" gap="0.001"); each variant carries the group's cases that use it and is one launch of one world per case.

The acceptance rule (accept()) is the project's reference-sensitivity policy: a case is compared when the oracle's own answer moves by less than SENS_MAX under
a one-ulp jitter of its fp32 input; a compared case has to agree within BOUND."""
import os
import struct
import tempfile

import numpy as np

from gymnasium_robotics_amd.mjcf import compile_mjcf

BOUND = 1e-4        # north-star bound of tests/test_gpu_tolerance_table.py
SENS_MAX = 1e-5     # a case is compared when the oracle moves less than this under the jitter: a tenth of the bound
DRAWS = 48          # jitter re-runs per case

PRIMS = ("sphere", "capsule", "box", "ellipsoid", "cylinder")
MESHES = ("ico12", "ico42")
CONDIMS = (1, 3, 4, 6)
_SIZE = {"sphere": "0.05", "capsule": "0.03 0.07", "box": "0.05 0.04 0.03", "ellipsoid": "0.06 0.04 0.03", "cylinder": "0.04 0.05"}
_SIZE_B = {"sphere": "0.065", "capsule": "0.035 0.09", "box": "0.07 0.05 0.04", "ellipsoid": "0.05 0.07 0.04", "cylinder": "0.055 0.04"}     # B differs from A: no pair is symmetric
_BPOS = np.array([0.3, -0.2, 0.4])      # off the world origin: the routines must work on differences of geom positions


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# meshes: faces known by construction
def _icosahedron():
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    return v / np.linalg.norm(v[0]), f


def _subdivide(v, f):
    v, mid, out = [tuple(p) for p in v], {}, []

    def m(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            p = np.array(v[a]) + np.array(v[b])
            v.append(tuple(p / np.linalg.norm(p)))
            mid[key] = len(v) - 1
        return mid[key]

    for a, b, c in f:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return np.array(v), out


def mesh_vertices(name):
    """(vertices, faces) of the two convex test meshes: a 12-vertex icosahedron of radius 6 cm (the small-mesh plane routine, <= 32 vertices) and its once-subdivided
    42-vertex icosphere scaled to 7 x 5 x 4 cm (the hull routine, > 32 vertices).  Points of an ellipsoid: every vertex is a hull vertex."""
    v, f = _icosahedron()
    if name == "ico12":
        return 0.06 * v, f
    v, f = _subdivide(v, f)
    return v * np.array([0.07, 0.05, 0.04]), f


def write_stl(path, name):
    v, f = mesh_vertices(name)
    with open(path, "wb") as fh:
        fh.write(b"\0" * 80 + struct.pack("<I", len(f)))
        for tri in f:
            fh.write(struct.pack("<3f", 0, 0, 0) + b"".join(struct.pack("<3f", *v[k]) for k in tri) + b"\0\0")


def compile_xml(xml):
    with tempfile.TemporaryDirectory() as d:
        for name in MESHES:
            if f'file="{name}.stl"' in xml:
                write_stl(os.path.join(d, name + ".stl"), name)
        p = os.path.join(d, "m.xml")
        with open(p, "w") as fh:
            fh.write(xml)
        return compile_mjcf(p)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# quaternions
def quat_mul(p, q):
    return np.array([p[0] * q[0] - p[1:] @ q[1:], *(p[0] * q[1:] + q[0] * p[1:] + np.cross(p[1:], q[1:]))])


def quat_rot(q, v):
    w, u = q[0], q[1:]
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


def axis_angle(axis, ang):
    axis = np.asarray(axis, dtype=np.float64)
    return np.r_[np.cos(ang / 2), np.sin(ang / 2) * axis / np.linalg.norm(axis)]


def quat_from_mat(R):
    """unit quaternion of a rotation matrix (the branch-free form is enough here: the test poses keep w well away from zero or are checked by the oracle's ncon)"""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-3:
        return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    k = int(np.argmax(np.diag(R)))
    i, j = (k + 1) % 3, (k + 2) % 3
    x = np.sqrt(max(0.0, 1.0 + R[k, k] - R[i, i] - R[j, j])) / 2.0
    q = np.zeros(4)
    q[0], q[1 + k], q[1 + i], q[1 + j] = (R[j, i] - R[i, j]) / (4 * x), x, (R[i, k] + R[k, i]) / (4 * x), (R[j, k] + R[k, j]) / (4 * x)
    return q


def _edge_across_edge():
    """box A (0.05 0.04 0.03) with its edge along local y at (-x, -z) laid across the top +y edge of box B (0.07 0.05 0.04, that edge runs along x), 1 mm deep: the
    edge of B is a ridge for the direction n = (0, 1, 1) / sqrt 2, A's edge runs along n x e_x, and A's centre sits on the ridge's normal"""
    n = np.array([0.0, 1.0, 1.0]) / np.sqrt(2.0)
    c = np.array([-0.05, 0.0, -0.03]); reach = np.linalg.norm(c); c /= reach
    ey = np.array([0.0, 1.0, 0.0])
    src = np.stack([c, ey, np.cross(c, ey)], axis=1)
    e = np.cross(n, [1.0, 0.0, 0.0])
    dst = np.stack([-n, e, np.cross(-n, e)], axis=1)
    q = quat_mul(quat_from_mat(dst @ src.T), axis_angle([0.3, 1.0, 0.2], 4e-4))
    return q, np.array([0.0103, 0.05, 0.04]) + n * (reach - 1e-3) + 2e-4 * e


def _unit(rng, n):
    x = rng.standard_normal(n)
    return x / np.linalg.norm(x)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
class Variant:
    """one compiled model and the cases that run on it: q0 [n, nq], v0 [n, nv], ctrl [n, max(nu, 1)] -- fp32 values held in fp64 -- and idx, each case's number in its group"""
    def __init__(self, xml, idx, q0, v0, ctrl=None):
        self.xml, self.idx = xml, list(idx)
        self.model = compile_xml(xml)
        self.nq, self.nv, self.nu = (self.model.dim(k) for k in ("nq", "nv", "nu"))
        self.q0, self.v0 = f32(q0).reshape(len(self.idx), self.nq), f32(v0).reshape(len(self.idx), self.nv)
        self.ctrl = f32(np.zeros((len(self.idx), max(self.nu, 1))) if ctrl is None else ctrl).reshape(len(self.idx), max(self.nu, 1))
        self.rk4 = self.model.dim("integrator") == 1
        self.want_contact = False      # True: the oracle must report a contact in every case; a list: in those cases


class Group:
    def __init__(self, name, kind, family, variants, cylinder_face=False):
        self.name, self.kind, self.family, self.variants, self.cylinder_face = name, kind, family, variants, cylinder_face
        self.n = sum(len(v.idx) for v in variants)


def _oracle(model):
    from oracle.oracle_sim import OracleSim

    return OracleSim(model)


def oracle_step(sim, q, v, ctrl):
    """one step of the live oracle from (q, v), zero warm start; returns x = (qpos | qvel) and (ncon, nefc) of the step"""
    sim.reset_data()
    sim.qpos[:], sim.qvel[:], sim.qacc_warmstart[:] = q, v, 0.0
    if sim.nu:
        sim.ctrl[:] = ctrl[:sim.nu]
    sim.step(1)
    return np.r_[sim.qpos, sim.qvel], (sim.ncon, sim.nefc)


def oracle_results(group, draws=DRAWS):
    """per variant: the oracle's x [n, nq + nv], (ncon, nefc) [n, 2] and its jitter sensitivity [n]: the largest change of x over `draws` re-runs in each of which every
    qpos component moves to a neighbouring fp32 value in a random direction.  The jitter generator is its own (seeded by the group's name and the case number), so the
    cases do not depend on the number of draws."""
    if draws in group.__dict__.setdefault("_oracle", {}):
        return group._oracle[draws]
    out = []
    for var in group.variants:
        sim = _oracle(var.model)
        n = len(var.idx)
        x, cnt, sens = np.zeros((n, var.nq + var.nv)), np.zeros((n, 2), dtype=np.int64), np.zeros(n)
        for i in range(n):
            x[i], cnt[i] = oracle_step(sim, var.q0[i], var.v0[i], var.ctrl[i])
            jit = np.random.default_rng([0x6A17, _name_seed(group.name), var.idx[i]])
            q32 = var.q0[i].astype(np.float32)
            for _ in range(draws):
                up = jit.integers(0, 2, var.nq).astype(bool)
                qj = np.where(up, np.nextafter(q32, np.float32(np.inf)), np.nextafter(q32, np.float32(-np.inf))).astype(np.float64)
                xj, _ = oracle_step(sim, qj, var.v0[i], var.ctrl[i])
                d = np.abs(xj - x[i]).max()
                sens[i] = max(sens[i], d if np.isfinite(d) else np.inf)
        assert sim.unsupported_hits == 0, (group.name, "the oracle has no routine for a pair of this model")
        want = range(n) if var.want_contact is True else var.want_contact or ()
        assert all(cnt[i, 0] > 0 for i in want), (group.name, "a case the oracle does not take", [var.idx[i] for i in want if cnt[i, 0] == 0])
        out.append((x, cnt, sens))
    group._oracle[draws] = out
    return out


def _name_seed(name):
    import zlib

    return zlib.crc32(name.encode())


def accept(group, device, oracle, min_share):
    """The acceptance rule, the same on the emulator and on the GPU.  device: per variant (x [n, nq + nv], status [n]); oracle: oracle_results(group).  Every case:
    finite output and a clean low status half.  Every COMPARED case (sensitivity < SENS_MAX): max |x_device - x_oracle| < BOUND.  At least min_share of the cases
    (a fraction, or a count when >= 1) must be compared.  Returns (compared, cases, worst error of the compared cases)."""
    compared, worst, bad = 0, 0.0, []
    for var, (xd, st), (xo, _, sens) in zip(group.variants, device, oracle):
        assert np.isfinite(xd).all(), (group.name, "non-finite output")
        assert (np.asarray(st) & 0xFFFF == 0).all(), (group.name, "status", [(var.idx[i], int(s)) for i, s in enumerate(st) if s & 0xFFFF])
        err = np.abs(xd - xo).max(axis=1)
        for i in range(len(var.idx)):
            if sens[i] < SENS_MAX:
                compared += 1
                worst = max(worst, err[i])
                if not err[i] < BOUND:
                    bad.append((var.idx[i], float(err[i]), float(sens[i])))
    print(f"{group.name}: compared {compared} / {group.n}, worst error {worst:.2e}")
    assert not bad, (group.name, "(case, error, oracle sensitivity) of the compared cases over the bound", bad)
    need = min_share if min_share >= 1 else min_share * group.n
    assert compared >= need - 1e-9, (group.name, f"only {compared} of {group.n} cases are well-posed for the oracle; {need} needed")
    return compared, group.n, worst


def min_share(group, record):
    """the caps: 90 % of a group's cases must be compared; a cylinder-face group, where the reference's portal search is ill-conditioned on the flat face, at least 10
    cases and no less than its recorded share (tests/golden/engine_matrix.json, from the oracle alone) minus 5 points"""
    if not group.cylinder_face:
        return 0.9
    return max(10.0, (record["groups"][group.name]["compared"] / group.n - 0.05) * group.n)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# A. pair groups
def _geom(kind, b=False):
    if kind in MESHES:
        return f'type="mesh" mesh="{kind}"'
    if kind == "plane":
        return 'type="plane" size="2 2 0.1"'
    return f'type="{kind}" size="{(_SIZE_B if b else _SIZE)[kind]}"'


def pair_xml(a, b, b_free, condim, margin, bquat):
    attrs = f'condim="{condim}" friction="0.8 0.02 0.002"' + (' margin="0.004" gap="0.001"' if margin else "")
    assets = "".join(f'<mesh name="{k}" file="{k}.stl"/>' for k in MESHES if k in (a, b))
    if b == "plane":
        bx = f'<geom {_geom(b)} {attrs}/>'
    elif b_free:
        bx = f'<body pos="{_BPOS[0]} {_BPOS[1]} {_BPOS[2]}"><freejoint/><geom {_geom(b, True)} mass="0.7" {attrs}/></body>'
    else:
        bx = f'<geom {_geom(b, True)} pos="{_BPOS[0]} {_BPOS[1]} {_BPOS[2]}" quat="{" ".join(repr(float(x)) for x in bquat)}" {attrs}/>'
    ax = f'<body pos="0 0 1"><freejoint/><geom {_geom(a)} mass="0.4" {attrs}/></body>'
    first, second = (ax, bx) if b_free else (bx, ax)
    return f'<mujoco><option timestep="0.002"/><asset>{assets}</asset><worldbody>{first}{second}</worldbody></mujoco>'


def pair_groups():
    """(name, a, b, b_free): A-plane for the seven types, every unordered pair of the five primitives with B static and with B free, each mesh against box, sphere
    and the other mesh with B static"""
    out = [(f"{a}-plane", a, "plane", False) for a in PRIMS + MESHES]
    for i, a in enumerate(PRIMS):
        for b in PRIMS[i:]:
            out += [(f"{a}-{b}-fixed", a, b, False), (f"{a}-{b}-free", a, b, True)]
    out += [(f"{m}-{b}-fixed", m, b, False) for m in MESHES for b in ("box", "sphere")] + [("ico12-ico42-fixed", "ico12", "ico42", False)]
    return out


def _cylinder_face(a, b):
    return (a == "cylinder" and b in ("sphere", "box", "cylinder")) or (b == "cylinder" and a in ("sphere", "box", "cylinder"))


def _case_variant(i):
    """condim cycles over 1, 3, 4, 6 (shifted by one every four cases, so the margin cases see all four); every fourth case has margin and gap"""
    return CONDIMS[(i + i // 4) % 4], i % 4 == 3


def _hand_placed(a, b):
    """poses next to the degenerate ones, as (quaternion of A in B's frame, position of A's centre in B's frame); each is a few 1e-4 off the exact pose, so the oracle
    stays continuous.  Sizes: _SIZE (A) and _SIZE_B (B)."""
    tilt = lambda ax, e: axis_angle(ax, e)
    if (a, b) == ("capsule", "capsule"):      # A: r 0.03 half 0.07; B: r 0.035 half 0.09
        return [(tilt([1, 0, 0], 3e-4), [0.0632, 0.0003, 0.011]),                  # near-parallel, overlapping along the axis (den <= GRX_MINVAL or next to it)
                (tilt([0, 1, 0], -2e-4), [0.0002, 0.0634, -0.052]),                # near-parallel, A's end beyond B's end: both clamps
                (tilt([1, 0, 0], 4e-4), [0.0003, -0.0002, 0.2235]),                # end to end: cap on cap along the common axis
                (tilt([1, 0, 0], np.pi / 2 + 3e-4), [0.035, 0.0003, 0.1434])]    # A across B's end: one clamp
    if (a, b) == ("capsule", "box"):          # B half sizes 0.07 0.05 0.04
        return [(quat_mul(tilt([0, 1, 0], np.pi / 2 + 3e-4), tilt([0, 0, 1], 2e-4)), [0.0003, 0.0002, 0.0688]),   # axis parallel to the top face: two contacts
                (quat_mul(tilt([0, 0, 1], 0.5), tilt([1, 0, 0], np.pi / 2 - 4e-4)), [0.0102, -0.0051, 0.0685]),     # the same, turned about the face normal
                (tilt([1, 0, 0], 3e-4), [0.0982, 0.0003, 0.0102])]                                                  # axis parallel to a side face and to an edge
    if (a, b) == ("sphere", "box"):           # A r 0.05
        return [(tilt([0, 0, 1], 0.3), [0.0112, 0.0053, 0.0367]),      # centre inside the box, nearest face +z
                (tilt([0, 0, 1], 0.3), [0.0665, 0.0103, -0.0051]),     # centre inside, nearest face +x
                (tilt([0, 0, 1], 0.3), [-0.0203, -0.0468, 0.0102]),    # centre inside, nearest face -y
                (tilt([0, 0, 1], 0.3), [0.0713, 0.0511, 0.0408])]      # centre just outside a corner
    if (a, b) == ("sphere", "sphere"):        # B r 0.065
        return [(tilt([0, 0, 1], 0.0), [3e-4, -2e-4, 2.5e-4]), (tilt([0, 0, 1], 0.0), [-1e-4, 3e-4, -4e-4])]       # nearly coincident centres
    if (a, b) == ("box", "box"):              # A 0.05 0.04 0.03 on B 0.07 0.05 0.04
        return [(tilt([1, 0, 0], 3e-4), [0.0052, -0.0031, 0.0688]),                                                  # face to face, aligned
                (quat_mul(tilt([0, 0, 1], np.pi / 4), tilt([1, 0, 0], 4e-4)), [0.0021, 0.0013, 0.0686]),             # face to face, turned by 45 degrees
                (quat_mul(tilt([0, 0, 1], np.pi / 2 + 2e-4), tilt([0, 1, 0], np.pi / 4 + 3e-4)), [0.0003, 0.0002, 0.0962]),   # A's edge (along B's x after the turn) on B's top face
                _edge_across_edge()]
    return []


def build_pair_group(spec, gidx):
    name, a, b, b_free = spec
    rng = np.random.default_rng([0xA11, _name_seed(name)])
    bquat = _unit(rng, 4) if b != "plane" else np.array([1.0, 0, 0, 0])
    n_random = 64 if _cylinder_face(a, b) else 40
    hand = _hand_placed(a, b)
    sims, cases = {}, {}

    def sim_of(key):
        if key not in sims:
            sims[key] = _oracle(compile_xml(pair_xml(a, b, b_free, key[0], key[1], bquat)))
        return sims[key]

    def state(qa, pa, qb):
        q = np.r_[pa, qa]
        return np.r_[q, _BPOS, qb] if b_free else q

    def touching(sim, q):
        sim.qpos[:], sim.qvel[:] = f32(q), 0.0
        sim.forward()
        return sim.ncon > 0

    for i in range(n_random + len(hand)):
        key = _case_variant(i)
        sim = sim_of(key)
        if i < n_random:
            qa, qb = _unit(rng, 4), (_unit(rng, 4) if b_free else bquat)
            d = np.array([0.0, 0.0, 1.0]) if b == "plane" else _unit(rng, 3)
            depth, vel = rng.uniform(3e-4, 3e-3), 0.3 * rng.standard_normal(12 if b_free else 6)
            base = np.zeros(3) if b == "plane" else _BPOS
            s = 0.4
            while not touching(sim, state(qa, base + s * d, qb)):       # walk in from far away to the outermost contact ...
                s -= 0.005
                assert s > -0.01, (name, i)
            lo, hi = s, s + 0.005
            for _ in range(32):                                         # ... and bisect the separation on the oracle's ncon
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if touching(sim, state(qa, base + mid * d, qb)) else (lo, mid)
            q = state(qa, base + (lo - depth) * d, qb)
        else:
            qrel, prel = hand[i - n_random]
            qb = _unit(rng, 4) if b_free else bquat
            vel = 0.3 * rng.standard_normal(12 if b_free else 6)
            q = state(quat_mul(qb, qrel), _BPOS + quat_rot(qb, np.asarray(prel, dtype=np.float64)), qb)
        cases.setdefault(key, []).append((i, q, vel))
    variants = []
    for key in sorted(cases):
        idx, q0, v0 = zip(*cases[key])
        var = Variant(pair_xml(a, b, b_free, key[0], key[1], bquat), idx, np.array(q0), np.array(v0))
        var.want_contact = True
        variants.append(var)
    family = "plane" if b == "plane" else "mesh" if a in MESHES else "cylinder-face" if _cylinder_face(a, b) else "convex" if {a, b} & {"ellipsoid", "cylinder"} else "analytic"
    return Group(name, "pair", family, variants, _cylinder_face(a, b))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# B. tree groups and C. solve-size groups
def _tree_xml(rng, joints, parents, integrator, free_first=False, fric=0.3, lim=0.4, actuators=True, extra_world="", extra_body=None, tail="", names=False):
    """joints: the joint type of each body; parents: index of the parent body (-1: the world).  Every joint gets a random axis and offset, armature, damping, sometimes a
    spring, friction loss on a share `fric` of the joints and limits on a share `lim`; every body a rotated box of random size (contype = conaffinity = 0).  names: body k is
    called b{k} (a weld refers to its bodies by name)."""
    kids = {k: [] for k in range(-1, len(joints))}
    for k, p in enumerate(parents):
        kids[p].append(k)
    act = []

    def body(k):
        jt = joints[k]
        pos = rng.uniform(-0.12, 0.12, 3) + (np.array([0.0, 0.0, 1.5]) if parents[k] < 0 else 0.0)
        if free_first and k == 0:
            j = "<freejoint/>"
        else:
            a = [f'name="j{k}" type="{jt}"', 'pos="{:.4f} {:.4f} {:.4f}"'.format(*rng.uniform(-0.03, 0.03, 3)), f'armature="{rng.uniform(0.002, 0.05):.4f}"', f'damping="{rng.uniform(0, 0.5):.4f}"']
            a.append('axis="{:.4f} {:.4f} {:.4f}"'.format(*_unit(rng, 3)))
            if rng.random() < 0.3:
                a.append(f'stiffness="{rng.uniform(0.5, 5):.4f}"' + f' springref="{0.3 * rng.standard_normal():.4f}"')
            if rng.random() < fric:
                a.append(f'frictionloss="{rng.uniform(0.05, 0.5):.4f}"')
            if rng.random() < lim:
                r = rng.uniform(0.05, 0.2) if jt == "slide" else rng.uniform(0.2, 0.6)
                a.append(f'limited="true" range="{-r * rng.uniform(0.5, 1):.4f} {r:.4f}"')
            j = f'<joint {" ".join(a)}/>'
            if actuators and rng.random() < 0.5:
                act.append(f'<motor joint="j{k}" gear="{rng.uniform(1, 5):.3f}"/>' if rng.random() < 0.5 else f'<position joint="j{k}" kp="{rng.uniform(5, 30):.3f}"/>')
        g = '<geom type="box" size="{:.4f} {:.4f} {:.4f}" pos="{:.4f} {:.4f} {:.4f}" quat="{:.5f} {:.5f} {:.5f} {:.5f}" mass="{:.4f}" contype="0" conaffinity="0"/>'.format(
            *rng.uniform(0.02, 0.08, 3), *rng.uniform(-0.05, 0.05, 3), *_unit(rng, 4), rng.uniform(0.1, 0.8))
        more = extra_body(k) if extra_body else ""
        return '<body{} pos="{:.4f} {:.4f} {:.4f}">'.format(f' name="b{k}"' if names else "", *pos) + j + g + more + "".join(body(c) for c in kids[k]) + "</body>"

    bodies = "".join(body(k) for k in kids[-1])
    return (f'<mujoco><compiler angle="radian"/><option timestep="{0.004 if integrator == "RK4" else 0.002}" integrator="{integrator}" gravity="1.5 -2 -9"/>'
            f'<worldbody>{extra_world}{bodies}{tail}</worldbody><actuator>{"".join(act)}</actuator></mujoco>')


def _states(rng, model, n, vscale, near_limits=False):
    """qpos0 perturbed by 0.3 N(0, 1) with the quaternions renormalised, qvel = vscale N(0, 1), ctrl = 0.5 N(0, 1).  near_limits: a limited hinge / slide joint is
    instead drawn inside its range (half of the time) or 0.3 .. 3 mm (mrad) beyond one of its ends -- the band the contacts of the pair groups are pressed in by"""
    nq, nv, nu = (model.dim(k) for k in ("nq", "nv", "nu"))
    t = model.tables
    jt, ja = np.asarray(t["jnt_type"]).reshape(-1), np.asarray(t["jnt_qposadr"]).reshape(-1)
    q = np.tile(np.asarray(t["qpos0"], dtype=np.float64).reshape(-1), (n, 1)) + 0.3 * rng.standard_normal((n, nq))
    if near_limits:
        lim, rng_ = np.asarray(t["jnt_limited"]).reshape(-1), np.asarray(t["jnt_range"], dtype=np.float64).reshape(-1, 2)
        for ty, adr, li, (lo, hi) in zip(jt, ja, lim, rng_):
            if ty in (2, 3) and li:
                for i in range(n):
                    u, over = rng.random(), rng.uniform(3e-4, 3e-3)
                    q[i, adr] = rng.uniform(lo, hi) if u < 0.5 else lo - over if u < 0.75 else hi + over
    for ty, adr in zip(jt, ja):
        if ty == 0:               # free
            s = adr + 3
            q[:, s:s + 4] /= np.linalg.norm(q[:, s:s + 4], axis=1, keepdims=True)
    return q, vscale * rng.standard_normal((n, nv)), 0.5 * rng.standard_normal((n, max(nu, 1)))


TREE_SETS = {"hs": ("hinge", "slide")}


def tree_groups():
    """(name, joint set, model number): Euler and RK4 in turn; models 2, 3, 6 and 7 start on a free joint (fast spin: the quaternion integration)"""
    return [(f"tree-{s}-{k}", s, k) for s in TREE_SETS for k in range(8)]


def build_tree_group(spec, gidx):
    name, jset, k = spec
    rng = np.random.default_rng([0xB22, _name_seed(name)])
    nb = int(rng.integers(2, 10))
    joints = [TREE_SETS[jset][int(rng.integers(len(TREE_SETS[jset])))] for _ in range(nb)]
    parents = [-1] + [int(rng.integers(0, i)) for i in range(1, nb)]
    xml = _tree_xml(rng, joints, parents, "RK4" if k % 2 else "Euler", free_first=k % 4 >= 2)
    model = compile_xml(xml)
    q, v, c = _states(rng, model, 6, 2.0)
    return Group(name, "tree", "tree-" + jset, [Variant(xml, range(6), q, v, c)])


SOLVE_NV = (13, 14, 15, 16, 21, 22, 24, 29, 30, 33, 36, 37)


def solve_groups():
    return [(f"solve-nv{n}", n, False) for n in SOLVE_NV] + [(f"solve-free-nv{n}", n, True) for n in (21, 30)]


def trailing_free_object(model):
    """the engine's own test for a trailing free object (grx_host_model.h): the last joint is a free joint of a child of the world that owns the last six dofs"""
    t = model.tables
    jt, jd, jb, par = (np.asarray(t[k]).reshape(-1) for k in ("jnt_type", "jnt_dofadr", "jnt_bodyid", "body_parent"))
    return len(jt) > 1 and model.dim("nv") > 6 and jt[-1] == 0 and jd[-1] == model.dim("nv") - 6 and par[jb[-1]] == 0


_R_LINK, _R_FREE = 0.05, 0.06


def build_solve_group(spec, gidx):
    """Hinge / slide trees of exactly nv dofs, branching (a parent among the three bodies before), limits on half of the joints and friction loss on half, so the Newton
    Hessian solve runs as well as the M + h B solve.  A limited joint sits inside its range or 0.3 .. 3 mm (mrad) beyond an end: 0.3 N(0, 1) about qpos0 would put
    it tens of centimetres past a 5 cm range, the limit rows would then change the velocities by ~10 per step, and an absolute bound of 1e-4 on a change of 10 asks
    for 1e-5 relative of a 30-dof fp32 solve -- a statement about the state, not about the solve.  Speeds are 0.5 N(0, 1), a quarter of the tree groups': these trees are up to 37 bodies deep and wide, the
    centripetal terms grow with the square of the tip speed, and this table is about the solve, not about the bias force.
    With a trailing free body (a sphere declared last; the robot has nv - 6 dofs): four states each with the sphere far from everything (M + h B and the Hessian block
    diagonal), resting on a static plane (contact rows, still block diagonal) and pressed 1 mm into the sphere of the robot's last link (linked: the full solve)."""
    name, nv, free = spec
    rng = np.random.default_rng([0xC33, _name_seed(name)])
    nb = nv - 6 if free else nv
    joints = ["hinge" if rng.random() < 0.7 else "slide" for _ in range(nb)]
    parents = [-1] + [int(rng.integers(max(0, i - 3), i)) for i in range(1, nb)]
    if not free:
        xml = _tree_xml(rng, joints, parents, "Euler", fric=0.5, lim=0.5)
        model = compile_xml(xml)
        assert model.dim("nv") == nv
        q, v, c = _states(rng, model, 6, 0.5, near_limits=True)
        return Group(name, "solve", "solve", [Variant(xml, range(6), q, v, c)])
    link = lambda k: f'<geom name="link" type="sphere" size="{_R_LINK}" mass="0.2" contype="0" conaffinity="1" condim="3"/>' if k == nb - 1 else ""
    plane = '<geom type="plane" size="3 3 0.1" contype="0" conaffinity="1" condim="3"/>'
    tail = f'<body pos="3 3 3"><freejoint/><geom name="ball" type="sphere" size="{_R_FREE}" mass="0.3" contype="1" conaffinity="0" condim="3"/></body>'
    xml = _tree_xml(rng, joints, parents, "Euler", fric=0.5, lim=0.5, extra_world=plane, extra_body=link, tail=tail)
    model = compile_xml(xml)
    assert model.dim("nv") == nv and trailing_free_object(model), (name, "the compiled model does not report the trailing free object: the case would test nothing")
    q, v, c = _states(rng, model, 12, 0.5, near_limits=True)
    sim = _oracle(model)
    for i in range(12):
        fq = q[i, -7:]
        if i < 4:
            fq[:3] = [3.0, 3.0, 3.0] + 0.1 * rng.standard_normal(3)
        elif i < 8:
            fq[:3] = [2.0 + 0.1 * rng.standard_normal(), -2.0, _R_FREE - 5e-4]
        else:
            sim.qpos[:], sim.qvel[:] = f32(q[i]), 0.0
            sim.forward()
            g = _link_geom(model)
            fq[:3] = sim.geom_xpos[3 * g:3 * g + 3] + (_R_LINK + _R_FREE - 1e-3) * _unit(rng, 3)
    var = Variant(xml, range(12), q, v, c)
    var.want_contact = list(range(4, 12))
    return Group(name, "solve", "solve-free", [var])


def _link_geom(model):
    """index of the robot's colliding sphere: the one geom of radius _R_LINK that is a sphere"""
    t = model.tables
    ty, sz = np.asarray(t["geom_type"]).reshape(-1), np.asarray(t["geom_size"], dtype=np.float64).reshape(-1, 3)
    hit = [g for g in range(len(ty)) if abs(sz[g, 0] - _R_LINK) < 1e-12 and sz[g, 1] == 0]
    assert len(hit) == 1, hit
    return hit[0]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# D. row groups: the rows and actuator forms the trees above never carry -- welds, joint equalities, fixed-tendon limits, affine actuators and their clamps, two
# actuators on one joint, impratio and noslip.  One compiled model per group (two for rows-options), ROWS_N cases each, no colliding geom unless the group says so.
ROWS_N = 7      # 6 .. 8 cases, never a multiple of 8 worlds
ROWS_GROUPS = ("rows-weld", "rows-jeq", "rows-tendon", "rows-actuator", "rows-mixed-euler", "rows-mixed-rk4", "rows-options")
_JEQ_POLY = (0.01, 0.8, -0.3, 0.2, -0.1)      # all five coefficients non-zero
_JEQ = ('<joint joint1="j{a}" joint2="j{b}" polycoef="' + " ".join(map(str, _JEQ_POLY)) + '" solimp="0.85 0.97 0.002 0.4 3"/>'       # five-value solimp, power 3
        '<joint joint1="j{c}" joint2="j{d}" polycoef="0 -1.2 0 0 0" solref="0.001 1"/>'      # solref[0] below two timesteps: the clamp
        '<joint joint1="j{e}" joint2="j{d}" active="false"/>')
# three fixed tendons with ranges of a few centimetres: one over two branches, one with margin and a negative solreflimit, one that lists a joint twice.  The joint
# named first is the one the states solve the tendon's length with (it belongs to no other tendon)
_TENDONS = ('<fixed limited="true" range="-0.03 0.04"><joint joint="j{a}" coef="1"/><joint joint="j{b}" coef="-0.7"/></fixed>'
            '<fixed limited="true" range="-0.025 0.035" margin="0.004" solreflimit="-1500 -50"><joint joint="j{c}" coef="1.2"/><joint joint="j{d}" coef="0.5"/></fixed>'
            '<fixed limited="true" range="-0.04 0.03"><joint joint="j{e}" coef="1"/><joint joint="j{f}" coef="0.6"/><joint joint="j{f}" coef="0.4"/></fixed>')
_TENDON_RANGE = ((-0.03, 0.04, 0.0), (-0.025, 0.035, 0.004), (-0.04, 0.03, 0.0))      # lower end, upper end, margin
# <general> with affine gain and bias, both clamps and a gear; <velocity>; <motor> with a ctrlrange; <position> plus <velocity> on ONE joint (the PD pair)
_ACTUATORS = ('<general joint="j{a}" gaintype="affine" gainprm="8 -3 0.5" biastype="affine" biasprm="0.4 -6 -0.8" ctrllimited="true" ctrlrange="-0.6 0.8" forcelimited="true" '
              'forcerange="-3 2.5" gear="2"/><velocity joint="j{b}" kv="1.5"/><motor joint="j{c}" ctrllimited="true" ctrlrange="-0.4 0.5" gear="3"/>'
              '<position joint="j{d}" kp="25"/><velocity joint="j{d}" kv="2"/>')
_CTRL_MODE = ((0, 1, 2, 0, 1, 2, 2), (2, 0, 1, 1, 0, 2, 2))      # per case: ctrl of the <general> / of the <motor> below (0), above (1) or inside (2) its ctrlrange
_WELD_QSTAR = np.array([0.4, 0.03, -0.5])      # the chain configuration whose tip pose the world weld holds


def rows_groups():
    return [(n,) for n in ROWS_GROUPS]


def _fmt(v):
    return " ".join(repr(float(x)) for x in v)


def _with(xml, k, attrs):
    """the text of _tree_xml with more attributes on joint j{k}"""
    key = f'name="j{k}" '
    assert xml.count(key) == 1
    return xml.replace(key, key + attrs + " ")


def _sections(xml, equality="", tendon="", actuator=""):
    assert xml.count("<actuator></actuator>") == 1
    return xml.replace("<actuator></actuator>", f"<equality>{equality}</equality><tendon>{tendon}</tendon><actuator>{actuator}</actuator>")


def _qadr(model, k):
    return int(np.asarray(model.tables["jnt_qposadr"]).reshape(-1)[model.names["joint"][f"j{k}"]])


def _dadr(model, k):
    return int(np.asarray(model.tables["jnt_dofadr"]).reshape(-1)[model.names["joint"][f"j{k}"]])


def _world_weld(xml, q, body):
    """a weld of a named body to the world, negative solref, with the explicit relpose that holds the body where it is at qpos = q (on the oracle): the world's pose in
    the body's frame"""
    model = compile_xml(xml)
    sim = _oracle(model)
    sim.qpos[:], sim.qvel[:] = f32(q), 0.0
    sim.forward()
    b = int(model.names["body"][body])
    x, r = sim.xpos[3 * b:3 * b + 3].copy(), sim.xquat[4 * b:4 * b + 4] * np.array([1.0, -1, -1, -1])
    return f'<weld body1="{body}" solref="-2000 -60" relpose="{_fmt(np.r_[quat_rot(r, -x), r])}"/>'


def _off(rng, n=None):
    """a few millimetres (milliradians) off, either way: a start 0.3 N(0, 1) away from a welded pose asks of the rows what build_solve_group's docstring says of limits"""
    return rng.uniform(3e-4, 3e-3, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)


def _poly(c, x):
    return c[0] + x * (c[1] + x * (c[2] + x * (c[3] + x * c[4])))


def _band(rng, lo, hi, margin, mode):
    """a coordinate inside [lo, hi] and clear of the margin (mode 0), or 0.3 .. 3 mm (mrad) beyond the lower (1) or the upper end (2): _states' near_limits, by turns"""
    over = rng.uniform(3e-4, 3e-3)
    return rng.uniform(lo + margin + 2e-3, hi - margin - 2e-3) if mode == 0 else lo - over if mode == 1 else hi + over


def _solve_tendons(rng, model, q, i, joints):
    """moves the first joint of each tendon of _TENDONS so that tendon t of case i is inside, below or above its range by turns: mode (i + t) % 3"""
    t_ = model.tables
    adr, num, qa, coef = (np.asarray(t_[k]).reshape(-1) for k in ("tendon_adr", "tendon_num", "wrap_qadr", "wrap_coef"))
    for t, (lo, hi, mg) in enumerate(_TENDON_RANGE):
        w = slice(adr[t], adr[t] + num[t])
        own = _qadr(model, joints[t])
        assert qa[w][0] == own and (qa[w] == own).sum() == 1
        rest = sum(c * q[a] for c, a in zip(coef[w][1:], qa[w][1:]))
        q[own] = (_band(rng, lo, hi, mg, (i + t) % 3) - rest) / coef[w][0]


def tendon_sides(var, i):
    """(lower active, upper active) of every tendon of the variant's model at case i, from the tables and the fp32 start alone, and the residuals of the active sides in
    the oracle's row order"""
    t_ = var.model.tables
    adr, num, qa = (np.asarray(t_[k]).reshape(-1) for k in ("tendon_adr", "tendon_num", "wrap_qadr"))
    coef, rg, mg = np.asarray(t_["wrap_coef"], dtype=np.float64).reshape(-1), np.asarray(t_["tendon_range"], dtype=np.float64).reshape(-1, 2), np.asarray(t_["tendon_margin"], dtype=np.float64).reshape(-1)
    sides, pos = [], []
    for t in range(len(adr)):
        ln = sum(coef[w] * var.q0[i, qa[w]] for w in range(adr[t], adr[t] + num[t]))
        d = (ln - rg[t, 0], rg[t, 1] - ln)
        sides.append((d[0] < mg[t], d[1] < mg[t]))
        pos += [x for x in d if x < mg[t]]
    return sides, np.array(pos)


def actuator_forces(var, i):
    """per actuator of case i, in numpy from the model tables: (ctrl, ctrlrange or None, unclamped force, forcerange or None, dof, generalised force gear * clamped force)"""
    t_ = var.model.tables
    g = lambda k, w=1: np.asarray(t_[k], dtype=np.float64).reshape(-1, w) if w > 1 else np.asarray(t_[k]).reshape(-1)
    trn, cl, fl, gt, bt, gear = g("act_trnid"), g("act_ctrllimited"), g("act_forcelimited"), g("act_gaintype"), g("act_biastype"), g("act_gear")
    cr, fr, gp, bp = g("act_ctrlrange", 2), g("act_forcerange", 2), g("act_gainprm", 3), g("act_biasprm", 3)
    ja, jd = g("jnt_qposadr"), g("jnt_dofadr")
    out = []
    for a in range(var.nu):
        ln, vel, u = gear[a] * var.q0[i, ja[trn[a]]], gear[a] * var.v0[i, jd[trn[a]]], var.ctrl[i, a]
        uc = min(cr[a, 1], max(cr[a, 0], u)) if cl[a] else u
        f = (gp[a, 0] + (gp[a, 1] * ln + gp[a, 2] * vel if gt[a] == 1 else 0.0)) * uc + (bp[a, 0] + bp[a, 1] * ln + bp[a, 2] * vel if bt[a] == 1 else 0.0)
        fc = min(fr[a, 1], max(fr[a, 0], f)) if fl[a] else f
        out.append((u, tuple(cr[a]) if cl[a] else None, f, tuple(fr[a]) if fl[a] else None, int(jd[trn[a]]), gear[a] * fc))
    return out


def _actuator_ctrl(rng, q, v, i, pd_q, pd_d):
    """ctrl of _ACTUATORS for case i: beyond either end of both ctrlranges by turns (_CTRL_MODE); on the shared joint a position error of 0.05 .. 0.5 and a velocity error
    of 0.1 .. 1, so that both of its actuators push with more than 0.05 (kp 25, kv 2)"""
    side = lambda lo, hi, mode: lo - rng.uniform(0.05, 0.4) if mode == 0 else hi + rng.uniform(0.05, 0.4) if mode == 1 else rng.uniform(lo, hi)
    sign = lambda: -1.0 if rng.random() < 0.5 else 1.0
    return np.array([side(-0.6, 0.8, _CTRL_MODE[0][i]), 0.5 * rng.standard_normal(), side(-0.4, 0.5, _CTRL_MODE[1][i]),
                     q[pd_q] + sign() * rng.uniform(0.05, 0.5), v[pd_d] + sign() * rng.uniform(0.1, 1.0)])


def _rows_weld(rng):
    """two free bodies welded to each other (torquescale, anchor) ahead of a hinge / slide / hinge chain whose tip is welded to the world (negative solref, explicit
    relpose).  The free pair moves as one by a random rigid motion per case; every welded pose is then left by a few millimetres and milliradians."""
    free = "".join(f'<body name="{n}" pos="{p}" quat="{_fmt(_unit(rng, 4))}"><freejoint/><geom type="box" size="{s}" mass="{m}" contype="0" conaffinity="0"/></body>'
                   for n, p, s, m in (("fa", "0.2 -0.1 0.3", "0.05 0.04 0.03", 0.4), ("fb", "0.32 -0.05 0.38", "0.04 0.06 0.03", 0.6)))
    base = _tree_xml(rng, ["hinge", "slide", "hinge"], [-1, 0, 1], "Euler", fric=0, lim=0, actuators=False, extra_world=free, names=True)
    q0 = np.asarray(compile_xml(base).tables["qpos0"], dtype=np.float64).reshape(-1)
    xml = _sections(base, equality='<weld body1="fa" body2="fb" solref="0.05 1" torquescale="0.7" anchor="0.02 -0.01 0.03"/>' + _world_weld(base, np.r_[q0[:14], _WELD_QSTAR], "b2"))
    q = np.zeros((ROWS_N, 17))
    for i in range(ROWS_N):
        r, t = _unit(rng, 4), 0.1 * rng.standard_normal(3)
        for s in (0, 7):
            q[i, s:s + 3] = quat_rot(r, q0[s:s + 3]) + t + _off(rng, 3)
            q[i, s + 3:s + 7] = quat_mul(quat_mul(r, q0[s + 3:s + 7]), axis_angle(_unit(rng, 3), _off(rng)))
        q[i, 14:] = _WELD_QSTAR + _off(rng, 3)
    return [Variant(xml, range(ROWS_N), q, 0.1 * rng.standard_normal((ROWS_N, 15)))]


def _rows_jeq(rng):
    """a branching tree; j2 (first branch) follows a quartic of j4 (second branch), j1 follows j3 through the solref clamp, the third equality is switched off"""
    xml = _sections(_tree_xml(rng, ["hinge", "hinge", "slide", "hinge", "hinge", "slide"], [-1, 0, 1, 0, 3, 0], "Euler", fric=0, lim=0, actuators=False),
                    equality=_JEQ.format(a=2, b=4, c=1, d=3, e=5))
    model = compile_xml(xml)
    q = 0.3 * rng.standard_normal((ROWS_N, 6))
    for i in range(ROWS_N):
        q[i, _qadr(model, 2)] = _poly(_JEQ_POLY, q[i, _qadr(model, 4)]) + _off(rng)
        q[i, _qadr(model, 1)] = -1.2 * q[i, _qadr(model, 3)] + _off(rng)
    return [Variant(xml, range(ROWS_N), q, 0.5 * rng.standard_normal((ROWS_N, 6)))]


def _rows_tendon(rng):
    xml = _sections(_tree_xml(rng, ["hinge", "slide", "hinge", "hinge", "slide", "hinge", "slide"], [-1, 0, 1, 0, 3, 0, 5], "Euler", fric=0, lim=0, actuators=False),
                    tendon=_TENDONS.format(a=2, b=4, c=1, d=5, e=6, f=3))
    model = compile_xml(xml)
    q = 0.3 * rng.standard_normal((ROWS_N, 7))
    for i in range(ROWS_N):
        _solve_tendons(rng, model, q[i], i, (2, 1, 6))
    return [Variant(xml, range(ROWS_N), q, 0.5 * rng.standard_normal((ROWS_N, 7)))]


def _rows_actuator(rng):
    xml = _sections(_tree_xml(rng, ["hinge", "slide", "hinge", "hinge", "hinge"], [-1, 0, 1, 0, 3], "Euler", fric=0, lim=0, actuators=False), actuator=_ACTUATORS.format(a=0, b=1, c=2, d=3))
    model = compile_xml(xml)
    q, v = 0.3 * rng.standard_normal((ROWS_N, 5)), 1.0 * rng.standard_normal((ROWS_N, 5))
    ctrl = np.array([_actuator_ctrl(rng, q[i], v[i], i, _qadr(model, 3), _dadr(model, 3)) for i in range(ROWS_N)])
    return [Variant(xml, range(ROWS_N), q, v, ctrl)]


_MIXED_PARENTS = [-1, 0, 1, -1, 3, 4, 3, 6, -1, 8, 8, 10, 9, 11]
_MIXED_JOINTS = ["hinge", "slide", "hinge", "hinge", "hinge", "slide", "hinge", "hinge", "hinge", "slide", "hinge", "hinge", "hinge", "slide"]
_MIXED = {}
_MIXED_LIMITS = {12: (-0.3, 0.4, 0.003), 13: (-0.06, 0.08, 0.002)}      # joint: lower end, upper end, margin


def rows_mixed(name, site=False):
    """(xml, qpos, qvel, ctrl) of rows-mixed-euler / rows-mixed-rk4: fourteen hinge / slide joints in three trees and a trailing free sphere, nv = 20 -- the register-resident
    solve and the MFMA Hessian with multi-entry rows that are no contact rows.  One world holds equality, friction-loss, joint-limit, tendon-limit and contact rows:
      tree 1  j0 j1 j2, the tip b2 welded to the world at _WELD_QSTAR (negative solref, explicit relpose)
      tree 2  j3 with the branches j4 j5 and j6 j7, whose tips b5 and b7 are welded to each other where qpos0 has them (torquescale, anchor): 6 rows over dofs 3 .. 7
      tree 3  j8 with j9 - j12 and j10 - j11 - j13; j9 follows a quartic of j11, j10 follows j3 through the solref clamp, a third equality is switched off
      tendons over j8 j1 (two trees), j11 j5 (margin, negative solreflimit) and j3 j6 j6; friction loss on j1, j9, j12, j13; limits with a margin on j12, j13
      the actuators of _ACTUATORS on j12, j13, j8 and the position / velocity pair on j3
      a free sphere, declared last, 0.5 mm inside a plane, condim 3
    site: a named site on b2, the tip of the first chain (tests/sim_dyn_cases.py)."""
    if (name, site) in _MIXED:
        return _MIXED[name, site]
    rng = np.random.default_rng([0xD44, _name_seed(name)])
    plane = '<geom type="plane" size="3 3 0.1" contype="0" conaffinity="1" condim="3"/>'
    tail = f'<body pos="2 -2 {_R_FREE}"><freejoint/><geom type="sphere" size="{_R_FREE}" mass="0.3" contype="1" conaffinity="0" condim="3"/></body>'
    tip = (lambda k: '<site name="tip" pos="0.03 0.01 0.05"/>' if k == 2 else "") if site else None
    base = _tree_xml(rng, _MIXED_JOINTS, _MIXED_PARENTS, "RK4" if name.endswith("rk4") else "Euler", fric=0, lim=0, actuators=False, extra_world=plane, extra_body=tip, tail=tail, names=True)
    for k, (lo, hi, mg) in _MIXED_LIMITS.items():
        base = _with(base, k, f'limited="true" range="{lo} {hi}" margin="{mg}"')
    for k, fl in ((1, 0.15), (9, 0.25), (12, 0.2), (13, 0.3)):
        base = _with(base, k, f'frictionloss="{fl}"')
    model = compile_xml(base)
    nq, nv = model.dim("nq"), model.dim("nv")
    qa, da = (lambda k: _qadr(model, k)), (lambda k: _dadr(model, k))
    qstar = np.zeros(nq)
    qstar[-4] = 1.0
    qstar[[qa(0), qa(1), qa(2)]] = _WELD_QSTAR
    xml = _sections(base, equality='<weld body1="b5" body2="b7" torquescale="0.7" anchor="0.02 -0.01 0.03"/>' + _world_weld(base, qstar, "b2") + _JEQ.format(a=9, b=11, c=10, d=3, e=8),
                    tendon=_TENDONS.format(a=8, b=1, c=11, d=5, e=3, f=6), actuator=_ACTUATORS.format(a=12, b=13, c=8, d=3))
    model = compile_xml(xml)
    q, v, ctrl = np.zeros((ROWS_N, nq)), 0.3 * rng.standard_normal((ROWS_N, nv)), np.zeros((ROWS_N, 5))
    for i in range(ROWS_N):
        for k in range(3):
            q[i, qa(k)] = _WELD_QSTAR[k] + _off(rng)
        for k in (4, 5, 6, 7):
            q[i, qa(k)] = _off(rng)
        for k in (3, 8, 11):
            q[i, qa(k)] = 0.3 * rng.standard_normal()
        _solve_tendons(rng, model, q[i], i, (8, 11, 3))
        q[i, qa(9)] = _poly(_JEQ_POLY, q[i, qa(11)]) + _off(rng)
        q[i, qa(10)] = -1.2 * q[i, qa(3)] + _off(rng)
        for n, (k, (lo, hi, mg)) in enumerate(_MIXED_LIMITS.items()):
            q[i, qa(k)] = _band(rng, lo, hi, mg, (i + n) % 3)
        q[i, -7:] = np.r_[2.0 + 0.1 * rng.standard_normal(), -2.0 + 0.1 * rng.standard_normal(), _R_FREE - 5e-4, _unit(rng, 4)]
        v[i, -6:] = 0.1 * rng.standard_normal(6)
        ctrl[i] = _actuator_ctrl(rng, q[i], v[i], i, qa(3), da(3))
    _MIXED[name, site] = (xml, q, v, ctrl)      # read only
    return _MIXED[name, site]


def _rows_mixed(name):
    xml, q, v, ctrl = rows_mixed(name)
    var = Variant(xml, range(ROWS_N), q, v, ctrl)
    assert 16 <= var.nv <= 24 and trailing_free_object(var.model), (name, "the compiled model does not report the trailing free object")
    var.want_contact = True
    return [var]


def _rows_options(rng):
    """a box on a plane, condim 4, gravity off the axis so that it slides: impratio="4" (cases 0 .. 3) and impratio="0.5" noslip_iterations="3" (cases 4 .. 6).  Poses as
    in the plane pair groups: the lowest corner 0 .. 2 mm deep, the box turned about the normal and tilted by 0.5 .. 3 mrad"""
    xml = lambda opt: (f'<mujoco><option timestep="0.002" gravity="1.5 -2 -9" {opt}/><worldbody><geom type="plane" size="2 2 0.1" condim="4" friction="0.8 0.02 0.002"/>'
                       '<body pos="0 0 1"><freejoint/><geom type="box" size="0.05 0.04 0.03" mass="0.4" condim="4" friction="0.8 0.02 0.002"/></body></worldbody></mujoco>')
    corners = np.array([[sx * 0.05, sy * 0.04, sz * 0.03] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    q, v = np.zeros((ROWS_N, 7)), 0.3 * rng.standard_normal((ROWS_N, 6))
    for i in range(ROWS_N):
        th = rng.uniform(0, 2 * np.pi)
        r = quat_mul(axis_angle([np.cos(th), np.sin(th), 0.0], rng.uniform(5e-4, 3e-3)), axis_angle([0, 0, 1], rng.uniform(-np.pi, np.pi)))
        low = min(quat_rot(r, c)[2] for c in corners)
        q[i] = np.r_[0.3 * rng.standard_normal(2), -low - rng.uniform(0.0, 2e-3), r]
    out = []
    for opt, idx in (('impratio="4"', range(0, 4)), ('impratio="0.5" noslip_iterations="3"', range(4, ROWS_N))):
        var = Variant(xml(opt), idx, q[list(idx)], v[list(idx)])
        var.want_contact = True
        out.append(var)
    return out


def build_rows_group(spec, gidx):
    name, = spec
    if name.startswith("rows-mixed"):
        return Group(name, "rows", "rows", _rows_mixed(name))
    rng = np.random.default_rng([0xD44, _name_seed(name)])
    variants = {"rows-weld": _rows_weld, "rows-jeq": _rows_jeq, "rows-tendon": _rows_tendon, "rows-actuator": _rows_actuator, "rows-options": _rows_options}[name](rng)
    assert all(var.nq >= 2 for var in variants)
    return Group(name, "rows", "rows", variants)


def oracle_rows(var):
    """per case, from one forward pass of the oracle at the start state: ncon, nefc, the row counts ne (equality), nf (friction loss), nl (limits, joint and tendon), ntl
    (tendon limits among them), the noslip sweeps taken, and the residuals efc_pos"""
    sim, out = _oracle(var.model), []
    for i in range(len(var.idx)):
        sim.reset_data()
        sim.qpos[:], sim.qvel[:], sim.qacc_warmstart[:] = var.q0[i], var.v0[i], 0.0
        if sim.nu:
            sim.ctrl[:] = var.ctrl[i][:sim.nu]
        sim.forward()
        row = {k: int(sim._L.orc_int(sim._h, k.encode())) for k in ("ncon", "nefc", "ne", "nf", "nl", "ntl")}
        out.append(dict(row, noslip_iter=int(sim.noslip_iter), pos=sim.efc("pos")))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
ALL = [("pair", s) for s in pair_groups()] + [("tree", s) for s in tree_groups()] + [("solve", s) for s in solve_groups()] + [("rows", s) for s in rows_groups()]
NAMES = [s[0] for _, s in ALL]
_BUILT = {}


def group(name):
    """the group of that name, built once per process"""
    if name not in _BUILT:
        gidx = NAMES.index(name)
        kind, spec = ALL[gidx]
        _BUILT[name] = {"pair": build_pair_group, "tree": build_tree_group, "solve": build_solve_group, "rows": build_rows_group}[kind](spec, gidx)
    return _BUILT[name]
