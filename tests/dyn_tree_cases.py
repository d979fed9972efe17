"""Generated kinematic trees for tests/test_cpu_dyn_trees.py and tests/test_gpu_dyn_trees.py.  Each case OWNS a description -- plain dicts of bodies, joints, geoms, inertial
blocks and sites, spelled the way an MJCF file spells them -- and emits two things from it: the input of tests/dyn_refs.py (poses as unit quaternions, angles in radians,
mass, centre of mass and inertia per body) and an MJCF string for the compiler.  The two meet nowhere else: orientations are converted here from MuJoCo's documented meaning of
euler / eulerseq, axisangle, xyaxes, zaxis and fromto, inertias come from the closed forms of the solids and the parallel-axis theorem, default classes are resolved here.  No
helper of the compiler is called.  Every number is written to the MJCF with repr(), so both sides read the same doubles.

Geoms have contype = conaffinity = 0, there are no actuators, gravity is oblique.  Every case has a site on its deepest leaf and one on a joint-less child body.

Worlds: N = 5 (13 once, RUN13).  World 0 is qpos0 at rest; the others have joint values up to +-1.5 rad / +-0.3 m beyond ref and qvel = 3 N(0, 1) (a free body: a random
attitude and, where the case says so, 10 rad/s), rounded to fp32.  World i is the same for every N."""
import numpy as np

import dyn_refs as R

GRAVITY = (1.5, -2.0, -9.0)
TIMESTEP = 0.002
N_WORLDS = 5
RUN13 = "free-root-tree"      # the case that also runs with 13 worlds
MAX_BODIES, MAX_DOFS = 63, 64      # moving bodies / dofs of `full`: tests/test_cpu_dyn_trees.py::test_full_is_at_the_compilers_limits holds them to the compiler's own checks


def rd(x, n=4):
    return np.round(np.asarray(x, dtype=np.float64), n)


def _unit(rng, n):
    x = rng.standard_normal(n)
    return x / np.linalg.norm(x)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# orientation spellings -> unit quaternion (MuJoCo's documented meaning; angles in `scale` radians per written unit)
def _rot_quat(Rm):
    """unit quaternion of a rotation matrix (largest-component branch)"""
    t = np.array([1 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2], 1 + Rm[0, 0] - Rm[1, 1] - Rm[2, 2], 1 - Rm[0, 0] + Rm[1, 1] - Rm[2, 2], 1 - Rm[0, 0] - Rm[1, 1] + Rm[2, 2]])
    k = int(np.argmax(t))
    s = 2.0 * np.sqrt(t[k])
    if k == 0:
        q = [s / 4, (Rm[2, 1] - Rm[1, 2]) / s, (Rm[0, 2] - Rm[2, 0]) / s, (Rm[1, 0] - Rm[0, 1]) / s]
    elif k == 1:
        q = [(Rm[2, 1] - Rm[1, 2]) / s, s / 4, (Rm[0, 1] + Rm[1, 0]) / s, (Rm[0, 2] + Rm[2, 0]) / s]
    elif k == 2:
        q = [(Rm[0, 2] - Rm[2, 0]) / s, (Rm[0, 1] + Rm[1, 0]) / s, s / 4, (Rm[1, 2] + Rm[2, 1]) / s]
    else:
        q = [(Rm[1, 0] - Rm[0, 1]) / s, (Rm[0, 2] + Rm[2, 0]) / s, (Rm[1, 2] + Rm[2, 1]) / s, s / 4]
    return R.unit(q)


def _z_to(v):
    """the smallest rotation that takes +z to v"""
    v = np.asarray(v, dtype=np.float64) / np.linalg.norm(v)
    ax = np.cross([0.0, 0.0, 1.0], v)
    s = np.linalg.norm(ax)
    if s < 1e-12:
        return np.array([1.0, 0, 0, 0]) if v[2] > 0 else np.array([0.0, 1.0, 0, 0])
    return R.qexp(np.arctan2(s, v[2]) * ax / s)


def ori_quat(ori, scale, eulerseq):
    if ori is None:
        return np.array([1.0, 0.0, 0.0, 0.0])
    kind, val = ori[0], np.asarray(ori[1], dtype=np.float64)
    if kind == "quat":
        return R.unit(val)
    if kind == "axisangle":
        return R.qexp(val[3] * scale * val[:3] / np.linalg.norm(val[:3]))
    if kind == "euler":      # lower-case letters: each rotation about an axis of the frame the ones before it produced, so the quaternions multiply on the right
        q = np.array([1.0, 0.0, 0.0, 0.0])
        for letter, a in zip(eulerseq, val):
            assert letter in "xyz"
            q = R.qmul(q, R.qexp(a * scale * np.eye(3)["xyz".index(letter)]))
        return R.unit(q)
    if kind == "xyaxes":
        x = val[:3] / np.linalg.norm(val[:3])
        y = val[3:] - (val[3:] @ x) * x
        y /= np.linalg.norm(y)
        return _rot_quat(np.stack([x, y, np.cross(x, y)], axis=1))
    if kind == "zaxis":
        return _z_to(val)
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# solids: (volume, inertia about the centre per unit density, in the solid's own frame)
def solid(kind, size):
    s = np.asarray(size, dtype=np.float64)
    if kind == "sphere":
        vol = 4.0 / 3.0 * np.pi * s[0] ** 3
        return vol, np.eye(3) * (2.0 / 5.0 * vol * s[0] ** 2)
    if kind == "box":
        a, b, c = s[:3]
        vol = 8.0 * a * b * c
        return vol, vol / 3.0 * np.diag([b * b + c * c, a * a + c * c, a * a + b * b])
    if kind == "ellipsoid":
        a, b, c = s[:3]
        vol = 4.0 / 3.0 * np.pi * a * b * c
        return vol, vol / 5.0 * np.diag([b * b + c * c, a * a + c * c, a * a + b * b])
    if kind == "cylinder":
        r, h = s[0], s[1]      # radius, half height
        vol = 2.0 * np.pi * r * r * h
        t = vol * (3.0 * r * r + 4.0 * h * h) / 12.0
        return vol, np.diag([t, t, vol * r * r / 2.0])
    if kind == "capsule":
        r, h = s[0], s[1]
        vc, (_, Ic) = 2.0 * np.pi * r * r * h, solid("cylinder", (r, h))
        vh = 2.0 / 3.0 * np.pi * r ** 3      # one half ball: centre of mass 3r/8 above its flat face, 83/320 m r^2 across and 2/5 m r^2 about the axis, about that centre
        t = 2.0 * (83.0 / 320.0 * vh * r * r + vh * (h + 3.0 * r / 8.0) ** 2)
        return vc + 2.0 * vh, Ic + np.diag([t, t, 2.0 * (2.0 / 5.0 * vh * r * r)])
    raise KeyError(kind)


def combine(parts):
    """(mass, centre, inertia about the centre) of parts [(mass, centre, inertia about its own centre, all in one frame)]: the parallel-axis theorem"""
    m = sum(p[0] for p in parts)
    c = sum(p[0] * np.asarray(p[1]) for p in parts) / m
    I = np.zeros((3, 3))
    for pm, pc, pI in parts:
        d = np.asarray(pc) - c
        I += pI + pm * ((d @ d) * np.eye(3) - np.outer(d, d))
    return m, c, I


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the description
def J(type, name, pos=(0, 0, 0), axis=(0, 0, 1), ref=0.0, armature=0.01, damping=0.1, stiffness=0.0, springref=0.0, cls=None, omit=()):
    """ref and springref of a hinge are in the case's angle unit; omit: the attributes a default class supplies (the values here are then the resolved ones)"""
    return dict(type=type, name=name, pos=rd(pos), axis=rd(axis), ref=float(ref), armature=float(armature), damping=float(damping), stiffness=float(stiffness), springref=float(springref),
                cls=cls, omit=tuple(omit))


def G(type, size, pos=(0, 0, 0), ori=None, density=1000.0, mass=None, fromto=None, cls=None, omit=()):
    return dict(type=type, size=rd(size), pos=rd(pos), ori=ori, density=float(density), mass=mass, fromto=None if fromto is None else rd(fromto), cls=cls, omit=tuple(omit))


def S(name, pos=(0, 0, 0), ori=None):
    return dict(name=name, pos=rd(pos), ori=ori)


def B(name, parent, pos=(0, 0, 0), ori=None, joints=(), geoms=(), inertial=None, sites=(), childclass=None):
    """parent: name of the parent body, None for the world.  inertial: dict(mass, pos, ori, diag [3]) or dict(mass, pos, full [xx yy zz xy xz yz])"""
    return dict(name=name, parent=parent, pos=rd(pos), ori=ori, joints=list(joints), geoms=list(geoms), inertial=inertial, sites=list(sites), childclass=childclass)


class Case:
    def __init__(self, name, seed, bodies, angle="radian", eulerseq="xyz", defaults="", vscale=3.0, spin=None):
        self.name, self.seed, self.bodies, self.angle, self.eulerseq, self.defaults, self.vscale, self.spin = name, seed, bodies, angle, eulerseq, defaults, vscale, spin
        self.scale = np.pi / 180.0 if angle == "degree" else 1.0
        self._tree = self._model = self._states = None
        names = [b["name"] for b in bodies]
        assert len(set(names)) == len(names) and all(b["parent"] is None or b["parent"] in names for b in bodies)
        self.bodies = []      # in the order of the file, depth first: the order of the body ids, the qpos words and the dofs

        def walk(parent):
            for b in bodies:
                if b["parent"] == parent:
                    self.bodies.append(b)
                    walk(b["name"])

        walk(None)
        assert len(self.bodies) == len(bodies)

    # -- the reference's input --------------------------------------------------------------------------------------------------------------------------
    def _geom_frame(self, g):
        """(size, pos, quat) of a geom: fromto puts the centre half way and the z axis along the segment"""
        if g["fromto"] is not None:
            p0, p1 = g["fromto"][:3], g["fromto"][3:]
            return np.array([g["size"][0], 0.5 * np.linalg.norm(p1 - p0), 0.0]), 0.5 * (p0 + p1), _z_to(p1 - p0)
        return g["size"], g["pos"], ori_quat(g["ori"], self.scale, self.eulerseq)

    def _inertia(self, b):
        if b["inertial"] is not None:
            i = b["inertial"]
            if "full" in i:
                f = np.asarray(i["full"], dtype=np.float64)
                return float(i["mass"]), np.asarray(i["pos"], dtype=np.float64), np.array([[f[0], f[3], f[4]], [f[3], f[1], f[5]], [f[4], f[5], f[2]]])
            Rm = R.qmat(ori_quat(i.get("ori"), self.scale, self.eulerseq))
            return float(i["mass"]), np.asarray(i["pos"], dtype=np.float64), Rm @ np.diag(np.asarray(i["diag"], dtype=np.float64)) @ Rm.T
        parts = []
        for g in b["geoms"]:
            size, pos, quat = self._geom_frame(g)
            vol, I = solid(g["type"], size)
            rho = g["mass"] / vol if g["mass"] is not None else g["density"]
            Rm = R.qmat(quat)
            parts.append((rho * vol, pos, Rm @ (rho * I) @ Rm.T))
        return combine(parts)

    @property
    def tree(self):
        if self._tree is None:
            idx = {b["name"]: k for k, b in enumerate(self.bodies)}
            out = []
            for b in self.bodies:
                m, c, I = self._inertia(b)
                joints = []
                for j in b["joints"]:
                    a = self.scale if j["type"] == "hinge" else 1.0
                    ax = np.asarray(j["axis"], dtype=np.float64)
                    joints.append(dict(type=j["type"], name=j["name"], pos=j["pos"], axis=ax / np.linalg.norm(ax), ref=j["ref"] * a, armature=j["armature"], damping=j["damping"],
                                       stiffness=j["stiffness"], springref=j["springref"] * a))
                out.append(dict(name=b["name"], parent=-1 if b["parent"] is None else idx[b["parent"]], pos=b["pos"], quat=ori_quat(b["ori"], self.scale, self.eulerseq), joints=joints,
                                mass=m, ipos=c, inertia=I, sites=[dict(name=s["name"], pos=s["pos"], quat=ori_quat(s["ori"], self.scale, self.eulerseq)) for s in b["sites"]]))
            self._tree = dict(gravity=GRAVITY, timestep=TIMESTEP, bodies=out)
        return self._tree

    # -- the MJCF ------------------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _num(v):
        return " ".join(repr(float(x)) for x in np.atleast_1d(v))

    def _ori_xml(self, ori):
        return "" if ori is None else f' {ori[0]}="{self._num(ori[1])}"'

    def _body_xml(self, k):
        b = self.bodies[k]
        out = [f'<body name="{b["name"]}" pos="{self._num(b["pos"])}"{self._ori_xml(b["ori"])}' + (f' childclass="{b["childclass"]}"' if b["childclass"] else "") + ">"]
        if b["inertial"] is not None:
            i = b["inertial"]
            tail = f'fullinertia="{self._num(i["full"])}"' if "full" in i else f'diaginertia="{self._num(i["diag"])}"{self._ori_xml(i.get("ori"))}'
            out.append(f'<inertial mass="{self._num(i["mass"])}" pos="{self._num(i["pos"])}" {tail}/>')
        for j in b["joints"]:
            if j["type"] == "free":
                out.append(f'<freejoint name="{j["name"]}"/>')
                continue
            a = dict(type=j["type"], pos=self._num(j["pos"]), axis=self._num(j["axis"]), ref=self._num(j["ref"]), armature=self._num(j["armature"]), damping=self._num(j["damping"]),
                     stiffness=self._num(j["stiffness"]), springref=self._num(j["springref"]))
            cls = f' class="{j["cls"]}"' if j["cls"] else ""
            out.append(f'<joint name="{j["name"]}"{cls} ' + " ".join(f'{n}="{v}"' for n, v in a.items() if n not in j["omit"]) + "/>")
        for g in b["geoms"]:
            nsize = {"sphere": 1, "capsule": 2, "cylinder": 2}.get(g["type"], 3)
            a = dict(type=g["type"], contype="0", conaffinity="0")
            if g["fromto"] is not None:
                a.update(size=self._num(g["size"][:1]), fromto=self._num(g["fromto"]))
            else:
                a.update(size=self._num(g["size"][:nsize]), pos=self._num(g["pos"]))
            a.update(mass=self._num(g["mass"])) if g["mass"] is not None else a.update(density=self._num(g["density"]))
            cls = f' class="{g["cls"]}"' if g["cls"] else ""
            out.append(f"<geom{cls} " + " ".join(f'{n}="{v}"' for n, v in a.items() if n not in g["omit"]) + (self._ori_xml(g["ori"]) if g["fromto"] is None else "") + "/>")
        for s in b["sites"]:
            out.append(f'<site name="{s["name"]}" pos="{self._num(s["pos"])}"{self._ori_xml(s["ori"])}/>')
        out += [self._body_xml(c) for c in range(len(self.bodies)) if self.bodies[c]["parent"] == b["name"]]
        return "".join(out) + "</body>"

    @property
    def xml(self):
        roots = "".join(self._body_xml(k) for k, b in enumerate(self.bodies) if b["parent"] is None)
        return (f'<mujoco><compiler angle="{self.angle}" eulerseq="{self.eulerseq}"/><option timestep="{TIMESTEP!r}" gravity="{self._num(GRAVITY)}"/>{self.defaults}'
                f"<worldbody>{roots}</worldbody></mujoco>")

    @property
    def model(self):
        if self._model is None:
            import engine_matrix_cases as C

            self._model = C.compile_xml(self.xml)
        return self._model

    # -- bookkeeping the comparisons need, from the description alone -----------------------------------------------------------------------------------------------
    def carrier(self, name):
        """the body a body is rigidly part of: itself if it has a joint, else the nearest ancestor that has one (None: the world)"""
        by = {b["name"]: b for b in self.bodies}
        while name is not None and not by[name]["joints"]:
            name = by[name]["parent"]
        return name

    @property
    def moving(self):
        return [b["name"] for b in self.bodies if b["joints"]]

    @property
    def site_names(self):
        return [s["name"] for b in self.bodies for s in b["sites"]]

    # -- the start states --------------------------------------------------------------------------------------------------------------------------------------
    def states(self, n):
        """dict(qpos [n, nq], qvel [n, nv]) of fp32-valued float64; world i does not depend on n"""
        tree = self.tree
        lay, nq, nv = R.layout(tree)
        q0 = R.qpos0(tree)
        q, v = np.tile(q0, (n, 1)), np.zeros((n, nv))
        for i in range(1, n):
            r = np.random.default_rng([0xD7E, self.seed, i])
            v[i] = self.vscale * r.standard_normal(nv)
            for b, k, qa, da in lay:
                t = tree["bodies"][b]["joints"][k]["type"]
                if t == "free":
                    q[i, qa:qa + 3] += r.uniform(-0.3, 0.3, 3)
                    quat = _unit(r, 4)
                    while abs(quat[0]) > 0.7:      # far from the identity
                        quat = _unit(r, 4)
                    q[i, qa + 3:qa + 7] = quat
                    if self.spin is not None:
                        v[i, da + 3:da + 6] = self.spin * _unit(r, 3)
                else:
                    q[i, qa] += r.uniform(-1.5, 1.5) if t == "hinge" else r.uniform(-0.3, 0.3)
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        return dict(qpos=f32(q), qvel=f32(v))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the cases
def _rand_joint(rng, name, jtype, arm=(0.01, 0.05)):
    spring = rng.random() < 0.3
    return J(jtype, name, pos=rng.uniform(-0.03, 0.03, 3), axis=_unit(rng, 3), ref=rd(rng.uniform(-0.5, 0.5) if jtype == "hinge" else rng.uniform(-0.1, 0.1)),
             armature=rd(rng.uniform(*arm)), damping=rd(rng.uniform(0.0, 0.5)), stiffness=rd(rng.uniform(0.5, 5.0)) if spring else 0.0, springref=rd(0.3 * rng.standard_normal()) if spring else 0.0)


def _rand_box(rng, lo=0.02, hi=0.06):
    return G("box", rng.uniform(lo, hi, 3), pos=rng.uniform(-0.04, 0.04, 3), ori=("quat", rd(_unit(rng, 4), 5)), density=rd(rng.uniform(500, 1500), 1))


def _rand_link(rng, name, parent, jtype, reach=0.12, arm=(0.01, 0.05), box=(0.02, 0.06), **kw):
    pos = rng.uniform(-reach, reach, 3) + (np.array([0.0, 0.0, 1.0]) if parent is None else 0.0)
    return B(name, parent, pos=pos, ori=("quat", rd(_unit(rng, 4), 5)), joints=[_rand_joint(rng, "j_" + name, jtype, arm)], geoms=[_rand_box(rng, *box)], **kw)


def _rand_fixed(rng, name, parent, site):
    """a joint-less child with a small box and a site"""
    return B(name, parent, pos=rng.uniform(-0.06, 0.06, 3), ori=("quat", rd(_unit(rng, 4), 5)), geoms=[_rand_box(rng, 0.01, 0.03)], sites=[S(site, rng.uniform(-0.03, 0.03, 3), ("quat", rd(_unit(rng, 4), 5)))])


def _rand_tree(name, seed, parents, reach=0.12, extra_joint_on=None, arm=(0.01, 0.05), box=(0.02, 0.06)):
    """body k hangs on parents[k] (-1: the world), hinge and slide joints drawn at random; a fixed child with a site on body 0 and a site on the deepest body"""
    rng = np.random.default_rng([0xD7C, seed])
    depth = [0] * len(parents)
    for k, p in enumerate(parents):
        depth[k] = 0 if p < 0 else depth[p] + 1
    leaf = max(range(len(parents)), key=lambda k: (depth[k], k))
    bodies, fixed = [], None
    for k, p in enumerate(parents):
        b = _rand_link(rng, f"b{k}", None if p < 0 else f"b{p}", "hinge" if rng.random() < 0.7 else "slide", reach=reach, arm=arm, box=box)
        if k == extra_joint_on:
            b["joints"].append(_rand_joint(rng, f"j_b{k}_2", "hinge", arm))
        if k == leaf:
            b["sites"].append(S("tip", rng.uniform(-0.03, 0.03, 3), ("quat", rd(_unit(rng, 4), 5))))
        bodies.append(b)
        if k == 0:
            fixed = _rand_fixed(rng, "fix0", "b0", "onfixed")
    return Case(name, seed, bodies + [fixed])


def _spellings():
    box = lambda *a, **k: G("box", *a, **k)
    bodies = [
        B("s0", None, pos=(0.1, -0.05, 1.0), ori=("euler", (35.0, -50.0, 20.0)), joints=[J("hinge", "h0", pos=(0.02, -0.03, 0.01), axis=(0.3, -0.2, 0.9), ref=25.0, damping=0.2)],
          geoms=[box((0.05, 0.03, 0.04), pos=(0.03, 0.01, -0.02), ori=("axisangle", (1.0, 2.0, -0.5, 40.0)), density=900.0)]),
        B("s1", "s0", pos=(0.12, 0.04, -0.06), ori=("axisangle", (0.2, -1.0, 0.4, 65.0)), joints=[J("hinge", "h1", pos=(-0.02, 0.01, 0.03), axis=(1.0, 0.5, 0.0), ref=-40.0, damping=0.1, stiffness=1.5, springref=10.0)],
          geoms=[box((0.03, 0.05, 0.02), pos=(-0.01, 0.03, 0.02), ori=("euler", (-20.0, 30.0, 75.0)), density=1100.0)]),
        B("s1f", "s1", pos=(0.03, -0.04, 0.05), ori=("euler", (80.0, 15.0, -35.0)), geoms=[box((0.02, 0.01, 0.03), ori=("zaxis", (0.3, -0.4, 0.8)), density=1300.0)],
          sites=[S("onfixed", (0.01, 0.02, -0.01), ("xyaxes", (0.5, 1.0, 0.2, -1.0, 0.3, 0.4)))]),
        B("s2", "s1", pos=(-0.05, 0.1, 0.07), ori=("xyaxes", (1.0, 0.4, -0.3, 0.2, 1.0, 0.5)), joints=[J("hinge", "h2", pos=(0.01, 0.02, -0.03), axis=(0.0, 0.6, -0.8), ref=55.0, damping=0.05)],
          geoms=[box((0.04, 0.02, 0.05), pos=(0.02, -0.02, 0.01), ori=("xyaxes", (0.1, 0.9, 0.3, -0.8, 0.2, 0.1)), density=800.0)]),
        B("s3", "s2", pos=(0.06, -0.08, 0.09), ori=("zaxis", (0.5, 0.3, -0.7)), joints=[J("hinge", "h3", pos=(-0.03, -0.01, 0.02), axis=(-0.7, 0.1, 0.4), ref=-15.0, damping=0.15)],
          geoms=[box((0.03, 0.03, 0.03), pos=(0.0, 0.02, 0.03), ori=("quat", (0.6, -0.3, 0.5, 0.2)), density=1000.0)], sites=[S("tip", (0.02, -0.03, 0.04), ("euler", (10.0, -70.0, 130.0)))]),
    ]
    return Case("spellings", 1, bodies, angle="degree", eulerseq="zyx")


def _multi_joint():
    rng = np.random.default_rng([0xD7C, 2])
    bodies = [
        B("m0", None, pos=(0.0, 0.1, 1.0), ori=("quat", (0.8, 0.2, -0.4, 0.3)), geoms=[_rand_box(rng)],
          joints=[J("slide", "m0x", pos=(0.01, 0.0, 0.02), axis=(1.0, 0.2, 0.0), ref=0.05, damping=0.3), J("slide", "m0y", pos=(0.0, 0.02, 0.0), axis=(-0.1, 1.0, 0.3), ref=-0.04, damping=0.2),
                  J("hinge", "m0r", pos=(0.03, -0.02, 0.04), axis=(0.2, 0.3, 1.0), ref=0.4, damping=0.1)]),
        B("m0c", "m0", pos=(0.1, 0.05, -0.08), ori=("quat", (0.9, -0.1, 0.3, 0.2)), joints=[J("hinge", "m0ch", pos=(0.02, 0.01, 0.0), axis=(0.0, 1.0, 0.2), ref=-0.3)], geoms=[_rand_box(rng)]),
        _rand_fixed(rng, "m0f", "m0c", "onfixed"),
        B("m1", None, pos=(0.4, -0.2, 1.1), ori=("quat", (0.5, 0.5, -0.6, 0.1)), geoms=[_rand_box(rng)],
          joints=[J("hinge", "m1a", pos=(0.04, 0.0, -0.02), axis=(1.0, 0.1, 0.0), ref=0.6, damping=0.1), J("hinge", "m1b", pos=(-0.03, 0.05, 0.02), axis=(0.1, -0.2, 1.0), ref=-0.5, damping=0.2, stiffness=2.0, springref=0.2)]),
        B("m1c", "m1", pos=(-0.06, 0.09, 0.1), ori=("quat", (0.7, 0.3, 0.1, -0.6)), joints=[J("slide", "m1cs", pos=(0.0, 0.01, 0.02), axis=(0.4, 0.4, 0.8), ref=0.03, damping=0.4)], geoms=[_rand_box(rng)]),
        B("m1d", "m1c", pos=(0.08, 0.02, 0.07), ori=("quat", (0.6, -0.5, 0.4, 0.3)), joints=[J("hinge", "m1dh", pos=(0.01, -0.02, 0.01), axis=(0.5, -0.5, 0.6), ref=0.2)], geoms=[_rand_box(rng)],
          sites=[S("tip", (0.03, 0.01, -0.02), ("quat", (0.4, 0.4, -0.7, 0.3)))]),
    ]
    return Case("multi-joint", 2, bodies)


def _principal_far(rng, diag):
    Rm = R.qmat(_unit(rng, 4))
    I = Rm @ np.diag(diag) @ Rm.T
    return rd([I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]], 6)


def _inertial():
    rng = np.random.default_rng([0xD7C, 3])
    tiny = lambda: G("sphere", (0.01,), mass=0.001)      # ignored: the body has an <inertial>
    bodies = [
        B("i0", None, pos=(0.0, 0.0, 1.0), ori=("quat", (0.9, 0.1, 0.3, -0.2)), joints=[J("hinge", "ih0", pos=(0.01, 0.02, 0.0), axis=(0.2, 1.0, 0.1), damping=0.05)], geoms=[tiny()],
          inertial=dict(mass=0.8, pos=rd((0.04, -0.03, 0.05)), ori=("quat", (0.5, 0.6, -0.4, 0.5)), diag=rd((0.004, 0.009, 0.012), 6))),
        B("i1", "i0", pos=(0.1, 0.05, 0.08), ori=("quat", (0.3, -0.7, 0.5, 0.4)), joints=[J("hinge", "ih1", pos=(-0.02, 0.0, 0.01), axis=(1.0, -0.3, 0.5), ref=0.3, damping=0.05)], geoms=[tiny()],
          inertial=dict(mass=0.6, pos=rd((-0.03, 0.05, 0.02)), full=_principal_far(rng, (0.002, 0.007, 0.008)))),
        _rand_fixed(rng, "i1f", "i1", "onfixed"),
        B("i2", "i1", pos=(-0.07, 0.1, 0.04), ori=("quat", (0.6, 0.2, -0.2, 0.7)), joints=[J("hinge", "ih2", pos=(0.0, 0.03, -0.02), axis=(-0.4, 0.2, 1.0), ref=-0.2, damping=0.05)], geoms=[tiny()],
          inertial=dict(mass=0.4, pos=rd((0.02, 0.02, -0.04)), full=_principal_far(rng, (0.001, 0.0035, 0.004))), sites=[S("tip", (0.05, -0.02, 0.03), ("quat", (0.1, 0.8, -0.5, 0.3)))]),
    ]
    return Case("inertial", 3, bodies, vscale=6.0)


def _density():
    rng = np.random.default_rng([0xD7C, 4])
    q = lambda: ("quat", rd(_unit(rng, 4), 5))
    bodies = [
        B("d0", None, pos=(0.0, 0.0, 1.0), ori=q(), joints=[J("hinge", "dh0", pos=(0.01, 0.0, 0.02), axis=(0.1, 0.2, 1.0), ref=0.2, damping=0.2)],
          geoms=[G("sphere", (0.05,), pos=(0.04, -0.02, 0.03), ori=q(), density=800.0), G("capsule", (0.025, 0.06), pos=(-0.05, 0.03, -0.02), ori=q(), density=1200.0)]),
        B("d1", "d0", pos=(0.12, 0.03, -0.05), ori=q(), joints=[J("slide", "ds1", pos=(0.0, 0.01, 0.0), axis=(0.3, 1.0, -0.2), ref=0.02, damping=0.3)],
          geoms=[G("cylinder", (0.03, 0.07), pos=(0.02, 0.04, 0.01), ori=q(), density=900.0)]),
        B("d2", "d1", pos=(-0.04, 0.1, 0.06), ori=q(), joints=[J("hinge", "dh2", pos=(0.02, -0.01, 0.0), axis=(1.0, 0.0, 0.4), ref=-0.4, damping=0.1)],
          geoms=[G("ellipsoid", (0.06, 0.03, 0.045), pos=(-0.03, 0.02, 0.05), ori=q(), density=1100.0)]),
        _rand_fixed(rng, "d2f", "d2", "onfixed"),
        B("d3", "d0", pos=(-0.1, -0.08, 0.04), ori=q(), joints=[J("hinge", "dh3", pos=(0.0, 0.02, 0.01), axis=(0.0, 1.0, 0.3), ref=0.5, damping=0.1)],
          geoms=[G("box", (0.05, 0.02, 0.035), pos=(0.03, -0.04, 0.02), ori=q(), density=700.0)]),
        B("d4", "d3", pos=(0.05, -0.1, 0.03), ori=q(), joints=[J("hinge", "dh4", pos=(-0.01, 0.0, 0.02), axis=(0.5, 0.5, 0.7), ref=-0.1, damping=0.1)],
          geoms=[G("capsule", (0.02,), fromto=(0.01, -0.02, 0.0, 0.09, 0.05, 0.11), density=1000.0)]),
        B("d5", "d4", pos=(0.09, 0.05, 0.11), ori=q(), joints=[J("slide", "ds5", pos=(0.0, 0.0, 0.01), axis=(0.2, -0.3, 1.0), ref=-0.03, damping=0.2)],
          geoms=[G("cylinder", (0.025, 0.04), pos=(0.01, 0.03, -0.02), ori=q(), mass=0.37)], sites=[S("tip", (0.02, 0.02, 0.05), q())]),
    ]
    return Case("density", 4, bodies)


def _fixed_children():
    rng = np.random.default_rng([0xD7C, 5])
    q = lambda: ("quat", rd(_unit(rng, 4), 5))
    bodies = [
        B("f0", None, pos=(0.0, 0.0, 1.0), ori=q(), joints=[J("hinge", "fh0", pos=(0.02, 0.0, -0.01), axis=(0.3, 1.0, 0.2), ref=0.3, damping=0.2)], geoms=[_rand_box(rng)]),
        B("f0a", "f0", pos=(0.08, -0.05, 0.06), ori=q(), geoms=[_rand_box(rng, 0.02, 0.05)]),      # no joint
        B("f0b", "f0a", pos=(-0.04, 0.09, 0.05), ori=q(), geoms=[_rand_box(rng, 0.02, 0.05)], sites=[S("onfixed", (0.02, -0.01, 0.03), q())]),      # no joint, two deep
        B("f1", "f0b", pos=(0.06, 0.04, -0.07), ori=q(), joints=[J("slide", "fs1", pos=(0.0, 0.01, 0.0), axis=(0.2, -0.4, 1.0), ref=0.04, damping=0.3)], geoms=[_rand_box(rng)]),
        B("f1a", "f1", pos=(0.05, 0.06, 0.04), ori=q(), geoms=[_rand_box(rng, 0.02, 0.04)], sites=[S("onfixed2", (0.0, 0.02, 0.01), q())]),
        B("f2", "f1a", pos=(-0.06, 0.03, 0.08), ori=q(), joints=[J("hinge", "fh2", pos=(0.01, 0.01, 0.02), axis=(1.0, 0.3, -0.2), ref=-0.5, damping=0.1)], geoms=[_rand_box(rng)],
          sites=[S("tip", (0.03, 0.0, -0.02), q())]),
        B("f0c", "f0", pos=(-0.07, 0.02, -0.05), ori=q(), geoms=[_rand_box(rng, 0.02, 0.04)]),      # a second fixed child of f0, listed behind a jointed subtree
    ]
    return Case("fixed-children", 5, bodies)


_DEFAULTS = ('<default><joint armature="0.03"/><default class="arm"><joint axis="0.0 1.0 0.3" damping="0.3" stiffness="2.0"/><geom density="700.0"/>'
             '<default class="wrist"><joint axis="1.0 0.0 0.2" damping="0.05"/><geom density="1500.0"/></default></default></default>')


def _defaults():
    rng = np.random.default_rng([0xD7C, 6])
    q = lambda: ("quat", rd(_unit(rng, 4), 5))
    box = lambda density, **k: G("box", rng.uniform(0.02, 0.05, 3), pos=rng.uniform(-0.04, 0.04, 3), ori=q(), density=density, **k)
    bodies = [
        B("a0", None, pos=(0.0, 0.0, 1.0), ori=q(), childclass="arm", geoms=[box(700.0, omit=("density",))],
          joints=[J("hinge", "ah0", pos=(0.01, 0.0, 0.02), axis=(0.0, 1.0, 0.3), ref=0.2, armature=0.03, damping=0.3, stiffness=2.0, omit=("axis", "armature", "damping", "stiffness"))]),
        B("a1", "a0", pos=(0.1, 0.03, 0.05), ori=q(), geoms=[box(1500.0, cls="wrist", omit=("density",)), box(950.0)],      # childclass inherited from a0; one geom names the nested class
          joints=[J("hinge", "ah1", pos=(0.0, 0.02, -0.01), axis=(1.0, 0.0, 0.2), ref=-0.3, armature=0.03, damping=0.05, stiffness=2.0, cls="wrist", omit=("axis", "armature", "damping", "stiffness"))]),
        _rand_fixed(rng, "a1f", "a1", "onfixed"),
        B("a2", "a1", pos=(-0.05, 0.08, 0.06), ori=q(), childclass="wrist", geoms=[box(1500.0, omit=("density",))],
          joints=[J("slide", "as2", pos=(0.0, 0.0, 0.01), axis=(1.0, 0.0, 0.2), ref=0.03, armature=0.008, damping=0.4, stiffness=2.0, omit=("axis", "stiffness"))]),      # its own armature and damping win
        B("a3", "a2", pos=(0.06, -0.04, 0.09), ori=q(), geoms=[box(700.0, cls="arm", omit=("density",))],
          joints=[J("hinge", "ah3", pos=(0.02, 0.01, 0.0), axis=(0.2, 0.9, -0.4), ref=0.1, armature=0.03, damping=0.05, stiffness=2.0, springref=0.4, omit=("armature", "damping", "stiffness"))],
          sites=[S("tip", (0.02, 0.03, -0.01), q())]),
    ]
    # the fixed child a1f carries explicit densities; it sits under childclass "arm", whose geom default only supplies what is omitted
    return Case("defaults", 6, bodies, defaults=_DEFAULTS)


def _free_body(rng, name, pos):
    free = J("free", "root_" + name, armature=0.0, damping=0.0)
    return B(name, None, pos=pos, ori=("quat", (0.3, -0.6, 0.5, 0.55)), joints=[free], geoms=[G("sphere", (0.01,), mass=0.001)],
             inertial=dict(mass=1.3, pos=rd((0.05, -0.04, 0.06)), full=_principal_far(rng, (0.004, 0.011, 0.013))))


def _free_root(alone):
    rng = np.random.default_rng([0xD7C, 7])
    q = lambda: ("quat", rd(_unit(rng, 4), 5))
    bodies = [_free_body(rng, "fr", (0.2, -0.1, 1.2)), _rand_fixed(rng, "frf", "fr", "onfixed")]
    bodies[0]["sites"].append(S("hub", (0.03, 0.02, -0.05), q()))
    if not alone:
        bodies += [
            B("fr1", "fr", pos=(0.1, 0.05, -0.04), ori=q(), joints=[J("hinge", "frh1", pos=(0.01, 0.0, 0.02), axis=(0.2, 1.0, 0.3), ref=0.3, armature=0.02, damping=0.1)], geoms=[_rand_box(rng)]),
            B("fr2", "fr1", pos=(0.06, -0.08, 0.07), ori=q(), joints=[J("slide", "frs2", pos=(0.0, 0.01, 0.0), axis=(1.0, -0.2, 0.4), ref=-0.02, armature=0.02, damping=0.3)], geoms=[_rand_box(rng)]),
            B("fr3", "fr2", pos=(-0.05, 0.04, 0.09), ori=q(), joints=[J("hinge", "frh3", pos=(0.0, 0.02, 0.01), axis=(-0.3, 0.4, 1.0), ref=-0.4, armature=0.02, damping=0.1)], geoms=[_rand_box(rng)],
              sites=[S("tip", (0.02, -0.03, 0.03), q())]),
        ]
    return Case("free-root-alone" if alone else "free-root-tree", 7 if alone else 8, bodies, spin=10.0)


def _two_trees():
    rng = np.random.default_rng([0xD7C, 9])
    free = _free_body(rng, "tf", (-0.5, 0.3, 1.4))
    arm = [_rand_link(rng, "t0", None, "hinge"), _rand_link(rng, "t1", "t0", "hinge"), _rand_fixed(rng, "t1f", "t1", "onfixed"), _rand_link(rng, "t2", "t1", "hinge")]
    arm[-1]["sites"].append(S("tip", (0.02, 0.01, 0.04), ("quat", (0.5, 0.1, -0.8, 0.3))))
    slider = _rand_link(rng, "ts", None, "slide")
    slider["sites"].append(S("onslider", (0.0, 0.02, 0.01)))
    return Case("two-trees", 9, [free] + arm + [slider])


def _full():
    """63 moving bodies and 64 dofs: a random tree whose body 5 has two joints.  Short, light links and armatures of 0.05 .. 0.1: with the links and armatures of the other
    trees (28 kg, cond(M) = 5e3) storing M and the right-hand side in fp32 alone moves qacc_smooth by 2.6e-5 of its scale, more than the 1e-5 the device is held to
    (fp32_conditioning below); with these it is 5e-6"""
    rng = np.random.default_rng([0xD7C, 10])
    parents = [-1] + [int(rng.integers(max(0, k - 6), k)) for k in range(1, MAX_BODIES)]
    return _rand_tree("full", 10, parents, reach=0.06, extra_joint_on=5, arm=(0.05, 0.1), box=(0.015, 0.04))


def _build():
    cases = [_spellings(), _multi_joint(), _inertial(), _density(), _fixed_children(), _defaults(), _free_root(True), _free_root(False)]
    cases += [_rand_tree(f"depth-{n}", 20 + n, list(range(-1, n - 1))) for n in (2, 3, 5, 9, 17)]
    cases += [_rand_tree("wide", 40, [-1] + [0] * 20), _full(), _two_trees()]
    return {c.name: c for c in cases}


CASES = _build()
NAMES = tuple(CASES)
RUNS = [(name, N_WORLDS) for name in NAMES] + [(RUN13, 13)]

_REF = {}


def reference(name, n):
    """the reference's answers for the n worlds of a case, stacked per field, with the error estimates under "err" (stacked the same way); computed once, read only"""
    if (name, n) not in _REF:
        case = CASES[name]
        st = case.states(n)
        rows = [R.evaluate(case.tree, st["qpos"][i], st["qvel"][i]) for i in range(n)]
        out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0] if k not in ("err", "site_names", "body_names")}
        out["site_names"], out["body_names"] = rows[0]["site_names"], rows[0]["body_names"]
        out["err"] = {k: np.stack([np.broadcast_to(np.asarray(r["err"][k], dtype=np.float64), np.shape(r[k])) for r in rows]) for k in rows[0]["err"] if k != "richardson"}
        out["richardson"] = [r["err"]["richardson"] for r in rows]
        _REF[(name, n)] = out
    return _REF[(name, n)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# what the compiled model keeps of the reference's bodies, and the reference's answer in the compiled model's rows
FORWARD_FIELDS = ("xpos", "xquat", "xipos", "site_xpos", "site_xmat", "site_jacp", "site_jacr", "M", "qfrc_bias", "qfrc_passive", "qfrc_smooth", "qacc_smooth", "qacc")
STEP_FIELDS = ("qpos1", "qvel1")

_WANT = {}


def want(name, n):
    """reference(name, n) re-indexed the way the compiled model is: body rows are the bodies that have a joint (a joint-less body is part of its carrier; row 0 is the world),
    xipos is the centre of mass of a carrier and everything it carries, site rows follow the compiled model's site ids.  Which body carries which comes from the description;
    the compiled model only says which row a NAME has.  Returns (fields, err), both {field: [n, ...]}."""
    if (name, n) not in _WANT:
        case, ref = CASES[name], reference(name, n)
        names = case.model.names
        assert set(names["body"]) == set(case.moving) | {"world"}, (sorted(names["body"]), case.moving)
        assert sorted(names["site"]) == sorted(case.site_names)
        row = {b: k for k, b in enumerate(ref["body_names"])}
        nb, ns = len(names["body"]), len(names["site"])
        mass = np.array([b["mass"] for b in case.tree["bodies"]])
        out, err = {}, {}
        for k, width in (("xpos", 3), ("xquat", 4), ("xipos", 3)):
            out[k], err[k] = np.zeros((n, nb, width)), np.zeros((n, nb, width))
        out["xquat"][:, 0, 0] = 1.0
        for b, r in names["body"].items():
            if b == "world":
                continue
            out["xpos"][:, r], out["xquat"][:, r] = ref["xpos"][:, row[b]], ref["xquat"][:, row[b]]
            part = [row[x["name"]] for x in case.bodies if case.carrier(x["name"]) == b]
            out["xipos"][:, r] = (mass[part][None, :, None] * ref["xipos"][:, part]).sum(axis=1) / mass[part].sum()
            for k in ("xpos", "xquat", "xipos"):
                err[k][:, r] = ref["err"][k][:, row[b]]
        order = [ref["site_names"].index(s) for s in sorted(names["site"], key=names["site"].get)]
        assert [names["site"][ref["site_names"][o]] for o in order] == list(range(ns))
        for k in ("site_xpos", "site_xmat", "site_jacp", "site_jacr", "site_xvelp", "site_xvelr"):
            out[k], err[k] = ref[k][:, order], ref["err"][k][:, order]
        out["site_xmat"], err["site_xmat"] = out["site_xmat"].reshape(n, ns, 9), err["site_xmat"].reshape(n, ns, 9)
        for k in ("M", "qfrc_bias", "qfrc_passive", "qfrc_smooth", "qacc_smooth", "qacc", "qpos1", "qvel1"):
            out[k], err[k] = ref[k], ref["err"][k]
        _WANT[(name, n)] = (out, err)
    return _WANT[(name, n)]


def joint_layout_matches(case):
    """the compiled model numbers joints, qpos words and dofs the way the description does"""
    t, names = case.model.tables, case.model.names["joint"]
    lay, nq, nv = R.layout(case.tree)
    assert (case.model.dim("nq"), case.model.dim("nv")) == (nq, nv)
    for k, (b, j, qa, da) in enumerate(lay):
        jn = case.tree["bodies"][b]["joints"][j]["name"]
        assert names[jn] == k and int(np.asarray(t["jnt_qposadr"]).reshape(-1)[k]) == qa and int(np.asarray(t["jnt_dofadr"]).reshape(-1)[k]) == da, jn


_ORACLE = {}


def oracle_run(name, n):
    """{field: [n, ...]}: OracleSim.forward() from each start for the forward fields, step(1) from the same start for qpos1 / qvel1; read only"""
    if (name, n) not in _ORACLE:
        from oracle.oracle_sim import OracleSim

        case = CASES[name]
        sim, st = OracleSim(case.model), case.states(n)
        ns, nv = sim.nsite, sim.nv
        rows = []
        for i in range(n):
            sim.reset_data()
            sim.qpos[:], sim.qvel[:], sim.qacc_warmstart[:] = st["qpos"][i], st["qvel"][i], 0.0
            sim.forward()
            assert sim.nefc == 0 and sim.ncon == 0 and sim.bad_state == 0 and sim.unsupported_hits == 0
            jp, jr = np.zeros((ns, 3, nv)), np.zeros((ns, 3, nv))
            for s in range(ns):
                jp[s], jr[s] = sim.jac_site(s)
            r = dict(xpos=sim.xpos.reshape(-1, 3).copy(), xquat=sim.xquat.reshape(-1, 4).copy(), xipos=sim.xipos.reshape(-1, 3).copy(), site_xpos=sim.site_xpos.reshape(-1, 3).copy(),
                     site_xmat=sim.site_xmat.reshape(-1, 9).copy(), site_jacp=jp, site_jacr=jr, M=sim.M.reshape(nv, nv).copy(), site_xvelp=jp @ sim.qvel, site_xvelr=jr @ sim.qvel,
                     **{k: getattr(sim, k).copy() for k in ("qfrc_bias", "qfrc_passive", "qfrc_smooth", "qacc_smooth", "qacc", "qfrc_constraint")})
            sim.reset_data()
            sim.qpos[:], sim.qvel[:], sim.qacc_warmstart[:] = st["qpos"][i], st["qvel"][i], 0.0
            sim.step(1)
            r.update(qpos1=sim.qpos.copy(), qvel1=sim.qvel.copy())
            rows.append(r)
        _ORACLE[(name, n)] = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    return _ORACLE[(name, n)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# conditioning: the precondition of tests/test_cpu_sim_dynamics.py, on the reference
VECTORS = ("qfrc_bias", "qfrc_passive", "qfrc_smooth", "qacc_smooth", "qacc")      # compared normalised by max(1, |the world's reference row|_inf), as sim_dyn_cases.error does
ABSOLUTE = ("xpos", "xquat", "xipos", "site_xpos", "site_xmat", "site_jacp", "site_jacr", "site_xvelp", "site_xvelr", "M", "qpos1", "qvel1")
DRAWS = 48
_SENS = {}


def measure(field, got, wantv):
    """worst error of one world's field in the measure it is compared in"""
    got, wantv = np.asarray(got, dtype=np.float64), np.asarray(wantv, dtype=np.float64)
    if not wantv.size:
        return 0.0
    d = float(np.abs(got - wantv).max())
    d = d if np.isfinite(d) else np.inf
    return d / max(1.0, float(np.abs(wantv).max())) if field in VECTORS else d


def reference_sensitivity(name, n, draws=DRAWS):
    """{field: [n]}: the largest change of the reference's own answer over `draws` re-evaluations in each of which every qpos word of the start moves to a neighbouring fp32
    value in a random direction (the jitter of sim_cases.oracle_sensitivity).  Both sides of a difference use two Richardson levels: their common truncation error cancels."""
    if (name, n, draws) not in _SENS:
        case = CASES[name]
        st = case.states(n)
        sens = {k: np.zeros(n) for k in VECTORS + ABSOLUTE}
        for i in range(n):
            jit = np.random.default_rng([0x6A17, case.seed, i])
            q32 = st["qpos"][i].astype(np.float32)
            base = R.evaluate(case.tree, st["qpos"][i], st["qvel"][i], levels=2)
            for _ in range(draws):
                up = jit.integers(0, 2, q32.size).astype(bool)
                qj = np.where(up, np.nextafter(q32, np.float32(np.inf)), np.nextafter(q32, np.float32(-np.inf))).astype(np.float64)
                got = R.evaluate(case.tree, qj, st["qvel"][i], levels=2)
                for k in sens:
                    g = R.sign_like(got[k], base[k]) if k == "xquat" else got[k]
                    sens[k][i] = max(sens[k][i], measure(k, g, base[k]) if k != "qpos1" else measure(k, g - qj, base[k] - st["qpos"][i]))
        _SENS[(name, n, draws)] = sens
    return _SENS[(name, n, draws)]


def fp32_conditioning(name, n):
    """{field: [n]}: how far qfrc_bias and qacc_smooth move, in the measure they are compared in, when nothing but the STORAGE of their inputs is fp32 -- one rounding, 2^-24
    relative, of every body's contribution to the bias, of every entry of M and of the right-hand side; first order, from the reference alone: |db| <= u sum_b |contribution_b|,
    |da| <= u |M^-1| (|M| |a| + |b|) componentwise.  No fp32 implementation can be held to less; a case whose figure reaches the bound tests the number format, not the engine."""
    u = 2.0 ** -24
    case, ref = CASES[name], reference(name, n)
    g = np.asarray(GRAVITY)
    mass = np.array([b["mass"] for b in case.tree["bodies"]])
    out = dict(qfrc_bias=np.zeros(n), qacc_smooth=np.zeros(n))
    for i in range(n):
        M, a, b = ref["M"][i], ref["qacc_smooth"][i], ref["qfrc_bias"][i]
        if not a.size:
            continue
        jp, jr, Iw, w = ref["com_jacp"][i], ref["com_jacr"][i], ref["Iw"][i], ref["com_vel"][i][1]
        # the bodies' shares of the bias as the reference forms them: gravity, and the rest (from b itself: b = sum of shares, so |b - gravity share| bounds what is left)
        grav = np.einsum("bki,bk->bi", jp, -mass[:, None] * g[None])
        gyro = np.einsum("bki,bk->bi", jr, np.cross(w, np.einsum("bkl,bl->bk", Iw, w)))
        rest = b - grav.sum(axis=0) - gyro.sum(axis=0)
        out["qfrc_bias"][i] = u * float((np.abs(grav).sum(axis=0) + np.abs(gyro).sum(axis=0) + np.abs(rest)).max()) / max(1.0, float(np.abs(b).max()))
        out["qacc_smooth"][i] = u * float((np.abs(np.linalg.inv(M)) @ (np.abs(M) @ np.abs(a) + np.abs(ref["qfrc_smooth"][i]))).max()) / max(1.0, float(np.abs(a).max()))
    return out
