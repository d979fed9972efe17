"""The narrow phase contact by contact (tests/test_cpu_contact_matrix.py on the lane emulator, tests/test_gpu_contact_matrix.py through grx.BatchedSim's contact outputs)
against the fp64 oracle's list, on top of tests/engine_matrix_cases.py (C) and tests/sim_contact_cases.py (K).  Plain Python and numpy.

a. the 42 pair groups of C as they are: each case is the start pose q0[i], v0[i] of its variant under forward(), so nothing lies between the pose and the list
b. seven rest-* groups: one geom on the plane at hand-placed poses that give SEVERAL contacts -- a box face down (4) and on an edge (2), a lying capsule (2), a cylinder
   flat on a cap and on its side, an icosahedron face down (3) and edge down (2), the 42-vertex hull face down with margin="0.004" gap="0.001" (hull neighbours inside
   the margin join) -- and rest-box-box: the four hand-placed box-box poses of C with depth and yaw draws around each.  Every pose is tilted a few 1e-4 rad off the
   exact one and pressed in by 0.3 .. 3 mm; condim cycles over 1 / 3 / 4 / 6 by C._case_variant.
   rest-ellipsoid is the exception to "several": a smooth body has ONE contact with a plane in both engines, whatever the pose.  The group holds the poses next to the
   three principal axes, where the support point moves fastest with the pose; its cases are asserted to have exactly one contact.
c. two crowd-* scenes for the driver of grx_collision, 5 worlds and 13 worlds (a launch that is no multiple of 8), every world perturbed by its own seeded draw:
   crowd-boxes: nine free boxes stacked and laid side by side on three static boxes and a plane -- nine box-box pairs in contact (more than one pass of the eight-pair
                queue) next to plane-box contacts, 52 .. 61 contacts: more than the default tables hold, within the re-run tables (64 contacts, 256 rows)
   crowd-mixed: all five primitives and both meshes, free and static (ten free bodies: the engine holds 64 dofs per world), 125 candidate pairs (the compaction sweep),
                and in every world a contact from each class of the driver: analytic, box-box queue, hull queue, general convex, small plane-mesh, large plane-mesh.
                The late queues append behind the analytic contacts, so the engine's list is NOT in pair order here: the order of the outputs is what is tested.
                (The class buckets of the sweep need more than 512 candidate pairs and more than 64 survivors of the broad phase; no scene here is that large.)
   The bodies are put down one after the other on the ORACLE (walk along a direction until its contact count rises, bisect, press in 1.5 mm); a world then turns every
   body about the vertical, tilts it by a few 1e-4 rad, shifts it sideways by up to a millimetre and changes its depth by up to a millimetre.

ACCEPTANCE (accept()).  A case is COMPARED when, over C.DRAWS one-ulp jitters of its fp32 qpos (the generator of C.oracle_results, seeded by group name and case number),
the oracle's contact set (geoms, dim, count, in its order) is unchanged and dist / pos / normal move by less than C.SENS_MAX: a condition on the reference from the
reference alone.  Every case: clean status, finite floats, the list in non-decreasing candidate-pair order.  Every compared case: equal count; after K.match equal geom
pairs (and dims, where the device reports them); dist / pos / normal within C.BOUND; the tangents within C.BOUND of K.make_frame of the DEVICE's normal in fp64 (the
rule switches at |n_y| = 0.5, and a comparison through the oracle's normal would be ill-posed next to the switch)."""
import numpy as np

import engine_matrix_cases as C
import sim_contact_cases as K

PAIR_NAMES = tuple(s[0] for kind, s in C.ALL if kind == "pair")
REST_NAMES = ("rest-capsule", "rest-box", "rest-ellipsoid", "rest-cylinder", "rest-ico12", "rest-ico42", "rest-box-box")
CROWD_NAMES = ("crowd-boxes", "crowd-mixed")
NAMES = PAIR_NAMES + REST_NAMES + CROWD_NAMES
CROWD_WORLDS = (5, 13)
RERUN_MAXCON, RERUN_MAXEFC = 64, 256      # core.RERUN_CAPACITY, asserted in the CPU file
CLASSES = ("analytic", "box-box", "hull", "convex", "plane-mesh-small", "plane-mesh-large")
_Z = np.array([0.0, 0.0, 1.0])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the oracle's list
def _sim(var):
    if "_contact_oracle" not in var.__dict__:
        var._contact_oracle = C._oracle(var.model)
    return var._contact_oracle


def _forward(var, q, v):
    """forward() of the variant's oracle at (q, v); the list in the ORACLE's order: contact_geom [n, 2], contact_dim [n], contact_dist [n], contact_pos [n, 3], normal [n, 3], nefc"""
    sim = _sim(var)
    sim.reset_data()
    sim.qpos[:], sim.qvel[:], sim.qacc_warmstart[:] = q, v, 0.0
    sim.forward()
    con = sim.contacts()
    assert len(con) == sim.ncon, "the oracle's list is longer than its reader holds"
    return dict(contact_geom=con[:, 7:9].astype(np.int64), contact_dim=con[:, 9].astype(np.int64), contact_dist=con[:, 0].copy(), contact_pos=con[:, 1:4].copy(),
                normal=con[:, 4:7].copy(), nefc=int(sim.nefc))


def oracle_list(var, i):
    """the oracle's contact list of case i of the variant, computed once: read only"""
    cache = var.__dict__.setdefault("_contact_lists", {})
    if i not in cache:
        cache[i] = _forward(var, var.q0[i], var.v0[i])
    return cache[i]


def oracle_sensitivity(group, draws=C.DRAWS):
    """per variant dict(same [n] bool, geometric [n]): over `draws` one-ulp jitters of qpos -- whether the contact set stayed what it was, and the largest change of
    dist / pos / normal"""
    if draws in group.__dict__.setdefault("_contact_sens", {}):
        return group._contact_sens[draws]
    out = []
    for var in group.variants:
        n = len(var.idx)
        same, geo = np.ones(n, dtype=bool), np.zeros(n)
        for i in range(n):
            base = oracle_list(var, i)
            jit = np.random.default_rng([0x6A17, C._name_seed(group.name), var.idx[i]])
            q32 = var.q0[i].astype(np.float32)
            for _ in range(draws):
                up = jit.integers(0, 2, var.nq).astype(bool)
                qj = np.where(up, np.nextafter(q32, np.float32(np.inf)), np.nextafter(q32, np.float32(-np.inf))).astype(np.float64)
                got = _forward(var, qj, var.v0[i])
                if any(got[k].shape != base[k].shape or (got[k] != base[k]).any() for k in ("contact_geom", "contact_dim")):
                    same[i] = False
                    break
                for k in ("contact_dist", "contact_pos", "normal"):
                    if got[k].size:
                        d = np.abs(got[k] - base[k]).max()
                        geo[i] = max(geo[i], d if np.isfinite(d) else np.inf)
        assert _sim(var).unsupported_hits == 0, (group.name, "the oracle has no routine for a pair of this model")
        out.append(dict(same=same, geometric=geo))
    group._contact_sens[draws] = out
    return out


def compared_mask(sens):
    return sens["same"] & (sens["geometric"] < C.SENS_MAX)


def counts(group):
    """(cases compared by the oracle's own sensitivity, multi-contact cases among them)"""
    compared = multi = 0
    for var, s in zip(group.variants, oracle_sensitivity(group)):
        m = compared_mask(s)
        compared += int(m.sum())
        multi += sum(1 for i in np.nonzero(m)[0] if len(oracle_list(var, int(i))["contact_dim"]) > 1)
    return compared, multi


def min_share(group, record):
    """the caps: 90 % of a group's cases are compared; a cylinder-face group at least 10 cases and no less than its recorded share (tests/golden/contact_matrix.json, from
    the oracle alone) minus 5 points"""
    if not group.cylinder_face:
        return 0.9
    return max(10.0, (record["groups"][group.name]["compared"] / group.n - 0.05) * group.n)


def accept(group, device, min_share, tangents):
    """The acceptance rule of the module docstring, the same on the emulator and on the GPU.  device: per variant a list over its cases of dict(status, ncon,
    contact_geom [n, 2], contact_dist [n], contact_pos [n, 3], normal [n, 3], and contact_dim [n], tangents [n, 6] where the device reports them).  Prints the worst
    error before it is asserted; returns (compared, multi-contact compared, worst error)."""
    sens = oracle_sensitivity(group)
    compared, multi, worst, worst_t, bad = 0, 0, 0.0, 0.0, []
    for var, dev, s in zip(group.variants, device, sens):
        mask = compared_mask(s)
        for i, got in enumerate(dev):
            tag = (group.name, var.idx[i])
            assert got["status"] & 0xFFFF == 0, (tag, "status", got["status"])
            n = got["ncon"]
            assert 0 <= n == len(got["contact_geom"]), (tag, "ncon", n)
            floats = [got[k] for k in ("contact_dist", "contact_pos", "normal") + (("tangents",) if tangents else ())]
            assert all(np.isfinite(f).all() for f in floats), (tag, "non-finite (a NaN is an element the launch did not write)")
            pairs = [K.pair_of(var.model, int(a), int(b)) for a, b in got["contact_geom"]]
            assert all(x <= y for x, y in zip(pairs, pairs[1:])), (tag, "the list is not in candidate-pair order", pairs)
            if not mask[i]:
                continue
            want = oracle_list(var, i)
            assert n == len(want["contact_dim"]), (tag, "ncon", n, len(want["contact_dim"]))
            perm = K.match(got["contact_geom"], got["contact_pos"], want)
            assert (got["contact_geom"][perm] == want["contact_geom"]).all(), tag
            if "contact_dim" in got:
                assert (got["contact_dim"][perm] == want["contact_dim"]).all(), (tag, "dim", got["contact_dim"][perm], want["contact_dim"])
            err = max([float(np.abs(got[k][perm].astype(np.float64) - want[k]).max()) for k in ("contact_dist", "contact_pos", "normal") if want[k].size] or [0.0])
            terr = 0.0
            if tangents and n:
                frames = np.array([K.make_frame(x) for x in got["normal"].astype(np.float64)])
                terr = float(np.abs(got["tangents"].astype(np.float64) - frames[:, 3:]).max())
            compared, multi = compared + 1, multi + (n > 1)
            worst, worst_t = max(worst, err), max(worst_t, terr)
            if not (err < C.BOUND and terr < C.BOUND):
                bad.append((var.idx[i], err, terr, float(s["geometric"][i])))
    print(f"{group.name}: compared {compared} / {group.n}, worst error {worst:.2e}, tangents {worst_t:.2e}, multi-contact {multi}")
    assert not bad, (group.name, "(case, error, tangent error, oracle sensitivity) of the compared cases over the bound", bad)
    need = min_share if min_share >= 1 else min_share * group.n
    assert compared >= need - 1e-9, (group.name, f"only {compared} of {group.n} cases are well-posed for the oracle; {need} needed")
    return compared, multi, worst


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# b. rest groups
def _down(d):
    """the rotation that takes the body direction d to straight down"""
    d = np.asarray(d, dtype=np.float64) / np.linalg.norm(d)
    c = -d[2]
    if c > 1.0 - 1e-12:
        return np.array([1.0, 0, 0, 0])
    if c < -1.0 + 1e-12:
        return C.axis_angle([1, 0, 0], np.pi)
    return C.axis_angle(np.cross(d, -_Z), np.arccos(c))


def _rest_pose(rng, d):
    """direction d down, turned about the vertical by any angle, then tilted by 2 .. 5e-4 rad about a horizontal axis"""
    th = rng.uniform(0, 2 * np.pi)
    tilt = C.axis_angle([np.cos(th), np.sin(th), 0.0], rng.uniform(2e-4, 5e-4) * (1 if rng.random() < 0.5 else -1))
    return C.quat_mul(tilt, C.quat_mul(C.axis_angle(_Z, rng.uniform(-np.pi, np.pi)), _down(d)))


def _ico_dirs(name):
    """(outward normals of the faces, directions of the edge midpoints) of a test mesh, in its own frame"""
    v, f = C.mesh_vertices(name)
    faces = [np.cross(v[b] - v[a], v[c] - v[a]) for a, b, c in f]
    faces = [n * np.sign(n @ (v[a] + v[b] + v[c])) for n, (a, b, c) in zip(faces, f)]
    edges = sorted({(min(a, b), max(a, b)) for tri in f for a, b in zip(tri, tri[1:] + tri[:1])})
    return faces, [v[a] + v[b] for a, b in edges]


def _rest_dirs(name):
    """per case the body direction that points down, and what the pose is called"""
    hx, hy, hz = 0.05, 0.04, 0.03
    if name == "rest-box":
        faces = [([0, 0, -1], "face"), ([0, 0, 1], "face"), ([1, 0, 0], "face"), ([0, -1, 0], "face"), ([-1, 0, 0], "face")]
        edges = [([hx, 0, -hz], "edge"), ([-hx, 0, hz], "edge"), ([0, hy, hz], "edge"), ([hx, -hy, 0], "edge"), ([0, -hy, -hz], "edge")]
        return faces + edges
    if name == "rest-capsule":
        return [([np.cos(a), np.sin(a), 0.0], "lying") for a in np.linspace(0.2, 5.8, 8)]
    if name == "rest-ellipsoid":
        return [(s * np.eye(3)[k], "axis") for k in range(3) for s in (1, -1)] + [([1, 1, 0], "between"), ([0, 1, -1], "between"), ([1, 0, 1], "between")]
    if name == "rest-cylinder":
        return [([0, 0, s], "cap") for s in (1, -1, 1, -1, 1)] + [([np.cos(a), np.sin(a), 0.0], "side") for a in np.linspace(0.3, 5.5, 5)]
    mesh = name[len("rest-"):]
    faces, edges = _ico_dirs(mesh)
    if mesh == "ico12":
        return [(faces[k], "face") for k in (0, 5, 11, 14, 19)] + [(edges[k], "edge") for k in (0, 7, 13, 21, 29)]
    return [(faces[k], "face") for k in (0, 9, 23, 38, 41, 57, 66, 79)]


def build_rest_group(name):
    """one geom of C._SIZE on the plane; the height comes from the oracle, as in C.build_pair_group: walk down to the first contact, bisect, press in 0.3 .. 3 mm"""
    rng = np.random.default_rng([0xE55, C._name_seed(name)])
    if name == "rest-box-box":
        return _build_rest_box_box(name, rng)
    a = name[len("rest-"):]
    sims, cases = {}, {}
    for i, (d, label) in enumerate(_rest_dirs(name)):
        cd, margin = C._case_variant(i)
        key = (cd, margin or a == "ico42")
        if key not in sims:
            sims[key] = C._oracle(C.compile_xml(C.pair_xml(a, "plane", False, key[0], key[1], None)))
        sim = sims[key]
        qa = _rest_pose(rng, d)

        def touching(z):
            sim.qpos[:], sim.qvel[:] = C.f32(np.r_[0.0, 0.0, z, qa]), 0.0
            sim.forward()
            return sim.ncon > 0

        s = 0.4
        while not touching(s):
            s -= 0.005
            assert s > -0.01, (name, i)
        lo, hi = s, s + 0.005
        for _ in range(32):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if touching(mid) else (lo, mid)
        q = np.r_[0.3 * rng.standard_normal(2), lo - rng.uniform(3e-4, 3e-3), qa]
        cases.setdefault(key, []).append((i, q, 0.3 * rng.standard_normal(6), label))
    variants, labels = [], {}
    for key in sorted(cases):
        idx, q0, v0, lab = zip(*cases[key])
        var = C.Variant(C.pair_xml(a, "plane", False, key[0], key[1], None), idx, np.array(q0), np.array(v0))
        var.want_contact = True
        variants.append(var)
        labels.update(zip(idx, lab))
    g = C.Group(name, "rest", "rest", variants)
    g.labels = labels
    return g


_BOX_BOX_AXES = ((_Z, 1.2e-3), (_Z, 1.4e-3), (_Z, 0.04 + (0.05 + 0.03) / np.sqrt(2.0) - 0.0962), (np.array([0.0, 1.0, 1.0]) / np.sqrt(2.0), 1e-3))
_BOX_BOX_LABELS = ("aligned", "turned", "edge-face", "edge-edge")


def _build_rest_box_box(name, rng):
    """C._hand_placed("box", "box") -- face on face aligned, turned by 45 degrees, edge on face, edge across edge -- and two draws around each: turned about the contact
    direction by 0.03 .. 0.2 rad either way, at a depth of 0.3 .. 3 mm.  _BOX_BOX_AXES: the contact direction in B's frame and the depth of the hand-placed pose."""
    bquat = C._unit(rng, 4)
    hand = C._hand_placed("box", "box")
    poses = []
    for k, (qrel, prel) in enumerate(hand):
        poses.append((np.asarray(qrel), np.asarray(prel, dtype=np.float64), _BOX_BOX_LABELS[k]))
        n, d0 = _BOX_BOX_AXES[k]
        for _ in range(2):
            yaw = rng.uniform(0.03, 0.2) * (1 if rng.random() < 0.5 else -1)
            poses.append((C.quat_mul(C.axis_angle(n, yaw), qrel), np.asarray(prel, dtype=np.float64) + n * (d0 - rng.uniform(3e-4, 3e-3)), _BOX_BOX_LABELS[k]))
    cases, labels = {}, {}
    for i, (qrel, prel, label) in enumerate(poses):
        key = C._case_variant(i)
        q = np.r_[C._BPOS + C.quat_rot(bquat, prel), C.quat_mul(bquat, qrel)]
        cases.setdefault(key, []).append((i, q, 0.3 * rng.standard_normal(6)))
        labels[i] = label
    variants = []
    for key in sorted(cases):
        idx, q0, v0 = zip(*cases[key])
        var = C.Variant(C.pair_xml("box", "box", False, key[0], key[1], bquat), idx, np.array(q0), np.array(v0))
        var.want_contact = True
        variants.append(var)
    g = C.Group(name, "rest", "rest", variants)
    g.labels = labels
    return g


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# c. crowd scenes
_ATTR = 'condim="3" friction="0.8 0.02 0.002"'
_X, _Y = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
_LYING = C.axis_angle([0, 1, 0], np.pi / 2)      # a capsule's or cylinder's axis along x


def _face_up(mesh, k):
    faces, _ = _ico_dirs(mesh)
    return _down(-faces[k])


def _crowd_spec(name):
    """(static geoms [(kind, pos, quat)], free bodies [dict(kind, xy, quat, steps [(direction, ...)], parent, yaw)]).  A free body starts above xy and is moved along
    each direction of `steps` in turn until it touches; parent: the body it rests on or against (its shifts carry over); yaw: the largest turn about the vertical a
    world may give it (a body laid against a vertical face keeps its face parallel to it within 5e-4 rad, like the hand-placed poses of C)."""
    one = np.array([1.0, 0, 0, 0])
    free = lambda kind, xy, quat=one, steps=(-_Z,), parent=None, yaw=0.2: dict(kind=kind, xy=np.asarray(xy, dtype=np.float64), quat=quat, steps=steps, parent=parent, yaw=yaw)
    if name == "crowd-boxes":
        xs = (-0.6, 0.0, 0.6)
        static = [("box", [x, 0.0, 0.04], one) for x in xs]
        bodies = []
        for k, x in enumerate(xs):
            bodies.append(free("box", [x + 0.004 * (k - 1), 0.003 * k]))                                    # 0 2 4: on the static box
            if k < 2:      # (a third box up there would take the worlds past the 64 contacts of the re-run tables)
                bodies.append(free("box", [x + 0.004 * (k - 1) + 0.003, 0.003 * k - 0.004], parent=2 * k))  # 1 3: on that one
        for k, x in enumerate(xs):
            bodies.append(free("box", [x + 0.16, 0.004 * (k - 1)], steps=(-_Z, -_X), yaw=5e-4))             # 5 6 7: on the plane, against the static box's +x face
        bodies.append(free("box", [0.0 + 0.12 + 0.14, 0.003], steps=(-_Z, -_X), parent=6, yaw=5e-4))        # 8: on the plane, against body 6
        return static, bodies
    static = [("box", [0.0, 0.0, 0.04], one), ("sphere", [0.4, 0.0, 0.065], one), ("capsule", [0.8, 0.0, 0.035], _LYING), ("ellipsoid", [0.0, 0.4, 0.04], one),
              ("cylinder", [0.4, 0.4, 0.08], C.axis_angle([0, 1, 0], 0.9)), ("ico12", [0.8, 0.4, 0.06], _face_up("ico12", 3)), ("ico42", [0.0, 0.8, 0.04], one)]
    bodies = [free("box", [0.004, -0.003]),                                               # 0: box on the static box                  box-box queue
              free("ellipsoid", [0.4005, 0.0005]),                                        # 1: ellipsoid on the static sphere         general convex
              free("capsule", [0.803, 0.002], quat=C.axis_angle([1, 0, 0], np.pi / 2)),   # 2: capsule across the static capsule      analytic
              free("ico42", [0.0005, 0.4005], quat=C.axis_angle([0.3, 1, 0.2], 0.7)),     # 3: 42-vertex hull on the static ellipsoid hull queue
              free("sphere", [0.397, 0.4005]),                                            # 4: sphere on the tilted cylinder's rim    general convex
              free("sphere", [0.802, 0.401]),                                             # 5: sphere on a face of the static ico12   hull queue
              free("box", [0.003, 0.802], quat=C.axis_angle([0.2, 1, 0.1], 0.25)),        # 6: box on the static hull                 hull queue
              free("ico12", [0.4, 0.8], quat=_down(_ico_dirs("ico12")[0][7])),            # 7: icosahedron face down on the plane     small plane-mesh
              free("ico42", [0.8, 0.8], quat=C.axis_angle([1, 0.4, 0.3], 1.1)),           # 8: 42-vertex hull on the plane            large plane-mesh
              free("cylinder", [1.2, 0.0], quat=C.axis_angle([1, 0, 0], np.pi / 2))]      # 9: cylinder on its side on the plane      analytic
    return static, bodies


def _crowd_xml(static, bodies):
    kinds = {k for k, _, _ in static} | {b["kind"] for b in bodies}
    assets = "".join(f'<mesh name="{k}" file="{k}.stl"/>' for k in C.MESHES if k in kinds)
    st = "".join(f'<geom {C._geom(k, True)} pos="{C._fmt(p)}" quat="{C._fmt(q)}" {_ATTR}/>' for k, p, q in static)
    fr = "".join(f'<body pos="0 0 {2 + k}"><freejoint/><geom {C._geom(b["kind"])} mass="0.4" {_ATTR}/></body>' for k, b in enumerate(bodies))
    return f'<mujoco><option timestep="0.002"/><asset>{assets}</asset><worldbody><geom {C._geom("plane")} {_ATTR}/>{st}{fr}</worldbody></mujoco>'


_NOMINAL_DEPTH = 1.5e-3


def _crowd_nominal(name, xml, bodies):
    """qpos of the scene with every body put down on the oracle, one after the other (the bodies not yet placed wait far apart, far away)"""
    sim = C._oracle(C.compile_xml(xml))
    q = np.zeros(7 * len(bodies))
    for k, b in enumerate(bodies):
        q[7 * k:7 * k + 7] = np.r_[50.0 + 3.0 * k, 50.0, 50.0, b["quat"] / np.linalg.norm(b["quat"])]

    def ncon(qq):
        sim.qpos[:], sim.qvel[:] = C.f32(qq), 0.0
        sim.forward()
        return sim.ncon

    for k, b in enumerate(bodies):
        q[7 * k:7 * k + 3] = np.r_[b["xy"], 0.45]
        for d in b["steps"]:
            base, s, qq = ncon(q), 0.0, q.copy()

            def at(s_):
                qq[7 * k:7 * k + 3] = q[7 * k:7 * k + 3] + s_ * d
                return ncon(qq)

            while at(s) <= base:
                s += 0.004
                assert s < 0.6, (name, k, "never touches")
            lo, hi = s - 0.004, s
            for _ in range(32):
                mid = 0.5 * (lo + hi)
                lo, hi = (lo, mid) if at(mid) > base else (mid, hi)
            q[7 * k:7 * k + 3] += (hi + _NOMINAL_DEPTH) * d
    return q


def _crowd_world(name, nominal, bodies, world):
    """world `world` of the scene: every body turned about the vertical through its centre (up to its yaw), tilted by 1 .. 4e-4 rad about a horizontal axis, shifted across
    its directions of approach by up to 1 mm and along each by up to 1 mm (a depth of 0.5 .. 2.5 mm); a body on or against another one follows that one's shift"""
    rng = np.random.default_rng([0xF66, C._name_seed(name), world])
    q, shift = nominal.copy(), []
    for k, b in enumerate(bodies):
        th = rng.uniform(0, 2 * np.pi)
        turn = C.quat_mul(C.axis_angle([np.cos(th), np.sin(th), 0.0], rng.uniform(1e-4, 4e-4)), C.axis_angle(_Z, rng.uniform(-b["yaw"], b["yaw"])))
        t = 1e-3 * rng.uniform(-1, 1, 3)
        t[2] = 0.0
        for d in b["steps"]:
            t = t - (t @ d) * d + 1e-3 * rng.uniform(-1, 1) * d
        t = t + (shift[b["parent"]] if b["parent"] is not None else 0.0)
        shift.append(t)
        q[7 * k:7 * k + 3] += t
        q[7 * k + 3:7 * k + 7] = C.quat_mul(turn, q[7 * k + 3:7 * k + 7])
    return q


def build_crowd_group(name):
    static, bodies = _crowd_spec(name)
    assert 6 * len(bodies) <= 64      # the engine's limit: 64 dofs per world
    xml = _crowd_xml(static, bodies)
    nominal = _crowd_nominal(name, xml, bodies)
    variants, first = [], 0
    for n in CROWD_WORLDS:      # the case numbers run on: 0 .. 4 in the launch of five worlds, 5 .. 17 in the launch of thirteen
        idx = range(first, first + n)
        q0 = np.array([_crowd_world(name, nominal, bodies, w) for w in idx])
        v0 = np.array([0.1 * np.random.default_rng([0xF67, C._name_seed(name), w]).standard_normal(6 * len(bodies)) for w in idx])
        var = C.Variant(xml, idx, q0, v0)
        var.want_contact = True
        variants.append(var)
        first += n
    return C.Group(name, "crowd", "crowd", variants)


def contact_class(model, g1, g2):
    """the class of grx_collision's driver a candidate pair belongs to, from the model tables: which routine or queue produces its contacts"""
    ty, mn = np.asarray(model.tables["geom_type"]).reshape(-1), np.asarray(model.tables["geom_meshnum"]).reshape(-1)
    (t1, a), (t2, b) = sorted([(int(ty[g1]), int(g1)), (int(ty[g2]), int(g2))])
    if t2 == 7:
        return "hull" if t1 != 0 else "plane-mesh-small" if mn[b] <= 32 else "plane-mesh-large"
    if t1 == 6 and t2 == 6:
        return "box-box"
    if t1 >= 2 and (t1 in (4, 5) or t2 in (4, 5)):
        return "convex"
    return "analytic"


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
_BUILT = {}


def group(name):
    """the group of that name, built once per process; a pair group is C's own object"""
    if name in PAIR_NAMES:
        return C.group(name)
    if name not in _BUILT:
        _BUILT[name] = build_crowd_group(name) if name in CROWD_NAMES else build_rest_group(name)
    return _BUILT[name]
