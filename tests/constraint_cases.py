"""Generated cases for the joint-space constraint rows, the actuators and RK4 (tests/test_cpu_constraint_refs.py, tests/test_cpu_constraint_rows.py,
tests/test_gpu_constraint_rows.py), on the generator of tests/dyn_tree_cases.py: a description, its MJCF and the input of tests/constraint_refs.py.  N = 5 worlds per case
(13 once, RUN13), seeded; world i is the same for every N.  Each case is named after its rows.

limits ......... hinge and slide limits on every joint: a margin with a five-value solimp, a solref below two timesteps, a negative solref, the defaults, by turns
friction ....... friction loss on every dof; two joints carry neither damping nor armature
tendons ........ three fixed tendons with limits: one over two branches, one with a margin and a negative solref, one that lists a joint twice
jeq ............ three joint equalities with quartic polycoef: a five-value solimp, a solref below two timesteps, one active="false"
actuators ...... <general> with gain, bias, gear and both clamps, <velocity>, <motor> with both clamps, <position> and <velocity> on ONE joint
mixed-8 ........ all kinds at nv = 8
mixed-20 ....... the same at nv = 20: the register-resident solve and the MFMA Hessian
free-root-rows . a free root carrying a limited arm with friction loss (short, light links, armatures of 0.05 .. 0.1): the free joint's averaged invweight0 and the arm's rows
                 meet in one M
rows-70 ........ 40 dofs, friction loss on every dof and 32 limited joints, 26 of which are beyond a range end in every world: nefc > 64, the first stride of the lane
                 loops; short, light links and armatures of 0.05 .. 0.1 as dyn_tree_cases' `full` (its fp32_conditioning lesson)
*-rk4 .......... limits, actuators and mixed-8 under RK4

States.  A limited joint or tendon of world i is inside its range (clear of the margin), below it or above it by 0.3 .. 3 mrad / mm, by turns over joints and worlds; a
friction dof has |qvel| of 1e-3 (it sticks) or 3 (it slips), by turns; an equality starts 0.3 .. 3 mrad off its curve; ctrl is below, above or inside a ctrlrange, and once
exactly ON a ctrlrange end and ON a forcerange end (a clamp is continuous: on the end both pieces give the same bits).  A state is redrawn (the draw count is recorded in
states()["draws"]) until, on the reference alone: every limit switch margin |dist - margin| >= 1e-4, every friction-zone margin and every clamp margin >= 1e-3 relative (or
exactly 0 for a clamp), the fp32-storage figures stay below half the vector bounds (fp32_storage: the inputs of the solve; fp32_inertia_storage: the bodies' inertias
about their tree's root, carried to qacc_smooth), and the reference's one-step answer moves by less than SENS_MAX over
engine_matrix_cases.DRAWS one-ulp jitters of the start (under RK4 its answer after RK4_STEPS = 3 steps too: three steps, not two).  tests/test_cpu_constraint_rows.py asserts
all of it again for every world of every case: none is left out anywhere."""
import json
import math
import os

import numpy as np

import constraint_refs as K
import dyn_refs as R
import dyn_tree_cases as T

N_WORLDS = 5
RUN13 = "mixed-8"
LIMIT_MARGIN, REL_MARGIN = 1e-4, 1e-3
SENS_MAX = 1e-5      # engine_matrix_cases.SENS_MAX (tests/test_cpu_constraint_rows.py checks that it is)
RK4_STEPS = 3      # step(RK4_STEPS) once per RK4 case
SOLIMP5 = (0.85, 0.97, 0.002, 0.4, 3.0)
POLY = (0.01, 0.8, -0.3, 0.2, -0.1)
VECTORS = ("qfrc_smooth", "qacc_smooth", "qfrc_constraint", "qacc", "qfrc_actuator")      # compared as sim_dyn_cases.error does: normalised by max(1, |the reference row|_inf)
MAX_DRAWS = 200


def vector_bounds():
    """test_gpu_sim_dynamics.vector_bounds() without that module's imports: the smallest power of ten >= 4 x the worst figure of the committed table"""
    import sim_dyn_cases as D

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim_dynamics_errors.json")) as fh:
        table = json.load(fh)["worst_error"]
    rows = [f"{s}/{k}/5" for s, k in D.CASES if s in D.BOUND_SCENES] + ["arm/1/13"]
    out = {}
    for f in D.VECTORS:
        worst = max(table[c][f] for c in rows)
        out[f] = 10.0 ** math.ceil(math.log10(4.0 * worst)) if worst > 0.0 else 0.0
    return out


def error(got, want):
    """one world's vector error in the measure of sim_dyn_cases.error"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not want.size:
        return 0.0
    d = float(np.abs(got - want).max())
    return (d if np.isfinite(d) else np.inf) / max(1.0, float(np.abs(want).max()))


class RowsCase(T.Case):
    """a Case whose states place every row on a chosen side of its switch.  limited: joint names; owners: the first joint of each tendon and joint1 of each equality (they
    belong to nothing else: the state solves the tendon's length / the equality's residual with them); ctrl_modes: per actuator the ctrl placement"""
    stick, always, ctrl_modes, _consts = (), frozenset(), (), None      # stick: friction joints that stick and slip by turns; always: limited joints never inside their range

    @property
    def consts(self):
        if self._consts is None:
            self._consts = K.constants(self.tree)
        return self._consts

    def forward(self, q, v, ctrl, levels=R.LEVELS):
        return K.forward(self.tree, q, v, ctrl, self.consts, levels)

    def step(self, q, v, ctrl, nstep=1, levels=R.LEVELS):
        return K.step(self.tree, q, v, ctrl, nstep, self.consts, levels)

    def _draw(self, i, draw):
        tree = self.tree
        jn, order = K.joints(tree)
        lay, nq, nv = R.layout(tree)
        r = np.random.default_rng([0xC0A5, self.seed, i, draw])
        q, v = R.qpos0(tree), self.vscale * r.standard_normal(nv)
        over = lambda: r.uniform(3e-4, 3e-3)

        def band(lo, hi, mg, mode):
            return r.uniform(lo + mg + 2e-3, hi - mg - 2e-3) if mode == 0 else lo - over() if mode == 1 else hi + over()

        for k, name in enumerate(order):
            j, qa, da = jn[name]
            if j["type"] == "free":
                q[qa:qa + 3] += r.uniform(-0.3, 0.3, 3)
                quat = T._unit(r, 4)
                while abs(quat[0]) > 0.7:
                    quat = T._unit(r, 4)
                q[qa + 3:qa + 7] = quat
                continue
            q[qa] += r.uniform(-1.0, 1.0) if j["type"] == "hinge" else r.uniform(-0.2, 0.2)
            if j.get("range") is not None:
                mode = (i + k) % 3 if name not in self.always else 1 + (i + k) % 2
                q[qa] = band(j["range"][0], j["range"][1], j.get("margin", 0.0), mode)
            if name in self.stick and (i + k) % 2 == 0:
                v[da] = 1e-3 * r.standard_normal()
        for t, ten in enumerate(tree.get("tendons", ())):
            (own, c0), rest = ten["joints"][0], ten["joints"][1:]
            want = band(ten["range"][0], ten["range"][1], ten.get("margin", 0.0), (i + t) % 3)
            q[jn[own][1]] = (want - sum(c * q[jn[n][1]] for n, c in rest)) / c0
        q0 = R.qpos0(tree)
        for e in tree.get("equalities", ()):
            if e.get("active", True):
                a1, a2 = jn[e["joint1"]][1], jn[e["joint2"]][1]
                x, c = q[a2] - q0[a2], e["polycoef"]
                q[a1] = q0[a1] + c[0] + x * (c[1] + x * (c[2] + x * (c[3] + x * c[4]))) + over() * (1.0 if r.random() < 0.5 else -1.0)
        f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
        q, v = f32(q), f32(v)
        ctrl = np.zeros(len(tree.get("actuators", ())))
        for a, act in enumerate(tree.get("actuators", ())):
            mode = self.ctrl_modes[a][i % len(self.ctrl_modes[a])]
            j, qa, da = jn[act["joint"]]
            if mode == "pd":      # a position / velocity target 0.05 .. 0.5 away
                ctrl[a] = (q[qa] if act["bias"][1] else v[da]) * act["gear"] + r.uniform(0.05, 0.5) * (1.0 if r.random() < 0.5 else -1.0)
            elif mode == "free":
                ctrl[a] = 0.5 * r.standard_normal()
            elif mode in ("below", "above", "inside"):
                lo, hi = act["ctrlrange"]
                ctrl[a] = lo - r.uniform(0.05, 0.4) if mode == "below" else hi + r.uniform(0.05, 0.4) if mode == "above" else r.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo))
                if mode == "inside" and act.get("forcerange") is not None:      # and the force inside its range, where a ctrl inside the ctrlrange gives one
                    flo, fhi = act["forcerange"]
                    u = (r.uniform(flo + 0.1 * (fhi - flo), fhi - 0.1 * (fhi - flo)) - act["bias"][0] - act["gear"] * (act["bias"][1] * q[qa] + act["bias"][2] * v[da])) / act["gain"]
                    ctrl[a] = u if lo + 0.05 * (hi - lo) < u < hi - 0.05 * (hi - lo) else ctrl[a]
            elif mode == "on-ctrl":
                ctrl[a] = act["ctrlrange"][1]
            elif mode == "on-force":      # a <motor>: force = ctrl
                ctrl[a] = act["forcerange"][1] / act["gain"]
            else:
                raise KeyError(mode)
        return q, v, f32(ctrl)

    def well_posed(self, world, q, v, ctrl, bounds):
        """(ok, figures) on the reference alone: the switch, zone and clamp margins, the fp32-storage figure and the one-ulp sensitivity (over RK4_STEPS steps too under RK4)"""
        f = self.forward(q, v, ctrl)
        lim = min([m[3] for m in f["margins"]["limit"]], default=np.inf)
        zone = min([z[1] for z in f["margins"]["zone"]], default=np.inf)
        clamp = min([(m[2] / max(1.0, abs(self._clamp_scale(m)))) for m in f["margins"]["clamp"] if m[2] != 0.0], default=np.inf)
        cond = dict(fp32_storage(f), qacc_smooth=fp32_inertia_storage(self.tree, q, f))
        fig = dict(limit=lim, zone=zone, clamp=clamp, **{"fp32_" + k: x for k, x in cond.items()})
        if not (lim >= LIMIT_MARGIN and zone >= REL_MARGIN and clamp >= REL_MARGIN and all(cond[k] < 0.5 * bounds[k] for k in cond)):
            return False, fig
        for nstep in (1,) + ((RK4_STEPS,) if self.integrator == "RK4" else ()):      # the dear ones last
            fig["sens%d" % nstep] = world_sensitivity(self, world, q, v, ctrl, nstep)
            if not fig["sens%d" % nstep] < SENS_MAX:
                return False, fig
        return True, fig

    def _clamp_scale(self, m):
        act = self.tree["actuators"][m[1]]
        return max(abs(x) for x in (act["ctrlrange"] if m[0] == "ctrl" else act["forcerange"]))

    def states(self, n, recorded=False):
        """dict(qpos [n, nq], qvel [n, nv], ctrl [n, nu]) of fp32-valued float64, draws [n] and figures [n]; world i does not depend on n.  recorded: take the draw the
        committed record names (tests/golden/constraint_rows_errors.json) without evaluating the preconditions again -- the device tests, which must stay quick;
        tests/test_cpu_constraint_rows.py asserts that the record is what the redraw loop gives"""
        if recorded:
            draws = recorded_draws()[self.name]
            st = [self._draw(i, draws[i] - 1) for i in range(n)]
            return dict(qpos=np.stack([s[0] for s in st]), qvel=np.stack([s[1] for s in st]), ctrl=np.stack([s[2] for s in st]).reshape(n, -1), draws=draws[:n])
        if self._states is None:
            self._states = {}
        bounds = vector_bounds()
        for i in range(n):
            if i not in self._states:
                for draw in range(MAX_DRAWS):
                    q, v, ctrl = self._draw(i, draw)
                    ok, fig = self.well_posed(i, q, v, ctrl, bounds)
                    if ok:
                        break
                else:
                    raise RuntimeError(f"{self.name}: world {i} met no precondition in {MAX_DRAWS} draws; change the case's parameters")
                self._states[i] = (q, v, ctrl, draw + 1, fig)
        st = [self._states[i] for i in range(n)]
        return dict(qpos=np.stack([s[0] for s in st]), qvel=np.stack([s[1] for s in st]), ctrl=np.stack([s[2] for s in st]).reshape(n, -1), draws=[s[3] for s in st],
                    figures=[s[4] for s in st])


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "constraint_rows_errors.json")


def recorded_draws():
    """{case: [draw count per world]} of the committed record"""
    with open(GOLDEN) as fh:
        return json.load(fh)["draws"]


def fp32_inertia_storage(tree, q, f):
    """how far qacc_smooth moves, first order and in the compared measure, when every body's spatial inertia ABOUT THE ORIGIN OF ITS TREE'S ROOT BODY -- rotational inertia,
    first moment and mass, the ten numbers a composite-rigid-body pass sums over a subtree -- is stored in fp32: |dM_ij| <= u sum_b |s_i|' |S_b| |s_j| over the bodies both
    dofs move, s the dof's motion (angular, linear at that origin), and |da| <= |M^-1| |dM| |a|.  About its own centre a light link's inertia is stored to 2^-24 of ITSELF;
    about a point r away it is stored to 2^-24 of m r^2, which is what a light hinge without armature then sees.  From the reference alone."""
    u = 2.0 ** -24
    kin = R.kinematics(tree, q)
    anc = R.ancestors(tree)
    nb, nv = len(tree["bodies"]), len(f["qacc_smooth"])
    root = [int(np.nonzero(anc[b])[0][0]) for b in range(nb)]      # parents come first: the first ancestor is the tree's root
    dM = np.zeros((nv, nv))
    for b in range(nb):
        O = kin["xpos"][root[b]]
        r, m, Iw = kin["xipos"][b] - O, tree["bodies"][b]["mass"], f["Iw"][b]
        S = np.zeros((6, 6))
        S[:3, :3] = Iw + m * ((r @ r) * np.eye(3) - np.outer(r, r))
        S[:3, 3:] = m * np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        S[3:, :3], S[3:, 3:] = S[:3, 3:].T, m * np.eye(3)
        dofs = [d for d in range(nv) if anc[b, kin["dof_body"][d]]]
        s = np.array([np.r_[kin["axis"][d], np.cross(kin["axis"][d], O - kin["anchor"][d])] if kin["kind"][d] == 1 else np.r_[np.zeros(3), kin["axis"][d]] for d in dofs]).reshape(len(dofs), 6)
        dM[np.ix_(dofs, dofs)] += u * np.abs(s) @ np.abs(S) @ np.abs(s).T
    a = f["qacc_smooth"]
    return float((np.abs(np.linalg.inv(f["M"])) @ (dM @ np.abs(a))).max()) / max(1.0, float(np.abs(a).max())) if nv else 0.0


def fp32_storage(f):
    """{field: figure}: how far qacc and qfrc_constraint move, in the compared measure, when the reference's own inputs to the solve (M, J, aref, D, a_s) are stored in fp32
    and the solve itself stays fp64"""
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
    rw = dict(kind=f["efc_kind"], J=f32(f["efc_J"]), aref=f32(f["efc_aref"]), D=f32(f["efc_D"]), R=1.0 / f32(f["efc_D"]) if f["nefc"] else np.zeros(0), floss=f["efc_floss"])
    M = f32(f["M"])
    sol = K.solve(0.5 * (M + M.T), f32(f["qacc_smooth"]), rw)
    fc = rw["J"].T @ sol["force"] if f["nefc"] else np.zeros_like(f["qacc"])
    return dict(qacc=error(sol["qacc"], f["qacc"]), qfrc_constraint=error(fc, f["qfrc_constraint"]))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _limit_rows(k, jtype):
    r = 0.4 if jtype == "hinge" else 0.1
    rows = dict(range=(-0.7 * r, r))
    v = k % 4
    if v == 0:
        rows.update(margin=0.01 if jtype == "hinge" else 0.004, solimplimit=SOLIMP5)
    elif v == 1:
        rows.update(solreflimit=(0.001, 1.0))      # below two timesteps
    elif v == 2:
        rows.update(solreflimit=(-1500.0, -50.0))
    return rows


def _case(name, seed, parents, limits=(), friction=(), bare=(), tendons=(), equalities=(), actuators=(), ctrl_modes=(), integrator="Euler", free_root=False, always=(),
          light=False, floss=(0.05, 0.5)):
    """a random tree (dyn_tree_cases._rand_tree) whose joints j_b{k} carry the rows asked for by index"""
    base = T._rand_tree(name, seed, parents, **(dict(reach=0.06, arm=(0.05, 0.1), box=(0.015, 0.04)) if light else {}))
    bodies = base.bodies
    rng = np.random.default_rng([0xC0A6, seed])
    if free_root:
        root = T._free_body(rng, "root", (0.2, -0.1, 1.2))
        root["inertial"]["pos"] = T.rd((0.01, -0.01, 0.02))      # the centre of mass near the joint: fp32_inertia_storage
        for b in bodies:
            if b["parent"] is None:
                b["parent"] = "root"
        bodies = [root] + bodies
    jt = {}
    for b in bodies:
        for j in b["joints"]:
            jt[j["name"]] = j
    jname = lambda k: f"j_b{k}"
    for k in limits:
        jt[jname(k)]["rows"].update(_limit_rows(k, jt[jname(k)]["type"]))
    for k in friction:
        jt[jname(k)]["rows"].update(frictionloss=float(T.rd(rng.uniform(*floss))))
        if k % 3 == 1:
            jt[jname(k)]["rows"].update(solreffriction=(0.03, 1.0), solimpfriction=(0.8, 0.9, 0.001, 0.5, 2.0))
    for k in bare:
        jt[jname(k)].update(damping=0.0, armature=0.0)
    case = RowsCase(name, seed, bodies, tendons=[dict(t, joints=[(jname(k), c) for k, c in t["joints"]]) for t in tendons],
                    equalities=[dict(e, joint1=jname(e["joint1"]), joint2=jname(e["joint2"])) for e in equalities],
                    actuators=[dict(a, joint=jname(a["joint"])) for a in actuators], integrator=integrator, timestep=0.004 if integrator == "RK4" else T.TIMESTEP)
    case.ctrl_modes, case.always, case.stick = list(ctrl_modes), {jname(k) for k in always}, {jname(k) for k in friction}
    return case


def _tendons(a, b, c, d, e, f):
    return [dict(joints=[(a, 1.0), (b, -0.7)], range=(-0.03, 0.04)),
            dict(joints=[(c, 1.2), (d, 0.5)], range=(-0.025, 0.035), margin=0.004, solref=(-1500.0, -50.0)),
            dict(joints=[(e, 1.0), (f, 0.6), (f, 0.4)], range=(-0.04, 0.03), solimp=SOLIMP5)]


def _equalities(a, b, c, d, e):
    return [dict(joint1=a, joint2=b, polycoef=POLY, solimp=SOLIMP5), dict(joint1=c, joint2=d, polycoef=(0.0, -1.2, 0.1, 0.0, 0.05), solref=(0.001, 1.0)),
            dict(joint1=e, joint2=d, polycoef=POLY, active=False)]


def _actuators(a, b, c, d):
    acts = [dict(tag="general", joint=a, gear=2.0, gain=8.0, bias=(0.4, -1.5, -0.2), ctrlrange=(-0.625, 0.75), forcerange=(-3.0, 2.5)), dict(tag="velocity", joint=b, kv=1.5),
            dict(tag="motor", joint=c, gear=3.0, ctrlrange=(-0.375, 0.625), forcerange=(-0.25, 0.5)), dict(tag="position", joint=d, kp=25.0), dict(tag="velocity", joint=d, kv=2.0)]
    modes = [("below", "above", "inside", "on-ctrl", "inside"), ("pd",), ("inside", "below", "above", "inside", "on-force"), ("pd",), ("pd",)]
    return acts, modes


_CHAIN8 = [-1, 0, 1, -1, 3, 4, 3, 6]
_TREE20 = [-1, 0, 1, -1, 3, 4, 3, 6, -1, 8, 8, 10, 9, 11, 2, 14, 5, 16, 7, 18]


def _build():
    acts4, modes4 = _actuators(0, 1, 2, 3)
    out = []
    for integ in ("Euler", "RK4"):
        tag = "" if integ == "Euler" else "-rk4"
        out.append(_case("limits" + tag, 101, [-1, 0, 1, 2, -1, 4], limits=range(6), integrator=integ))
        out.append(_case("actuators" + tag, 105, [-1, 0, 1, 2], actuators=acts4, ctrl_modes=modes4, integrator=integ))
        a8, m8 = _actuators(6, 7, 0, 3)
        out.append(_case("mixed-8" + tag, 106, _CHAIN8, limits=(0, 3, 7), friction=(0, 1, 5), tendons=_tendons(1, 0, 1, 0, 1, 0)[:1],
                         equalities=[dict(joint1=2, joint2=3, polycoef=POLY, solimp=SOLIMP5), dict(joint1=4, joint2=5, polycoef=(0.0, -1.2, 0.1, 0.0, 0.05), solref=(0.001, 1.0)),
                                     dict(joint1=6, joint2=5, polycoef=POLY, active=False)], actuators=a8, ctrl_modes=m8, integrator=integ, light=True))
    out.append(_case("friction", 102, [-1, 0, 1, -1, 3], friction=range(5), bare=(1, 4)))
    out.append(_case("tendons", 103, [-1, 0, 1, -1, 3, 4, 3], tendons=_tendons(0, 4, 1, 2, 3, 5), limits=(6,)))
    out.append(_case("jeq", 104, [-1, 0, 1, -1, 3, 4], equalities=_equalities(0, 3, 1, 4, 2)))
    a20, m20 = _actuators(15, 16, 17, 18)
    out.append(_case("mixed-20", 107, _TREE20, limits=(0, 3, 7, 9, 12, 13, 19), friction=(0, 1, 5, 8, 11, 14), tendons=_tendons(2, 0, 6, 3, 10, 9),
                     equalities=_equalities(4, 5, 11, 12, 14), actuators=a20, ctrl_modes=m20, light=True))
    out.append(_case("free-root-rows", 108, [-1, 0, 1], limits=(0, 1, 2), friction=(1, 2), free_root=True, light=True))
    rng = np.random.default_rng([0xC0A6, 70])
    parents70 = [-1] + [int(rng.integers(max(0, k - 6), k)) for k in range(1, 40)]
    out.append(_case("rows-70", 109, parents70, limits=range(32), always=range(6, 32), friction=range(40), light=True, floss=(0.02, 0.1)))
    return {c.name: c for c in out}


CASES = _build()
NAMES = tuple(CASES)
RK4 = tuple(n for n in NAMES if n.endswith("-rk4"))
RUNS = [(name, N_WORLDS) for name in NAMES] + [(RUN13, 13)]

_REF = {}


def reference(name, n, recorded=False):
    """per world the forward pass of the start, and qpos / qvel after one step (and after RK4_STEPS for an RK4 case); computed once, read only"""
    if (name, n) not in _REF:
        case = CASES[name]
        st = case.states(n, recorded)
        rows = []
        for i in range(n):
            q1, v1, f = case.step(st["qpos"][i], st["qvel"][i], st["ctrl"][i])
            f = dict(f, qpos1=q1, qvel1=v1)
            if name in RK4:
                f["qposk"], f["qvelk"], _ = case.step(st["qpos"][i], st["qvel"][i], st["ctrl"][i], nstep=RK4_STEPS)
            rows.append(f)
        _REF[(name, n)] = rows
    return _REF[(name, n)]


def stacked(name, n, field):
    return np.stack([np.asarray(r[field], dtype=np.float64) for r in reference(name, n)])


def world_sensitivity(case, world, q, v, u, nstep=1, draws=None):
    """the largest change of the reference's own answer (the vectors in their compared measure, qpos and qvel after nstep steps absolutely; nefc must not change) over
    `draws` one-ulp fp32 jitters of the start's qpos (the jitter of dyn_tree_cases.reference_sensitivity).  Both sides of a difference use two Richardson levels"""
    import engine_matrix_cases as C

    draws = C.DRAWS if draws is None else draws
    jit = np.random.default_rng([0x6A17, case.seed, world])
    q32 = np.asarray(q).astype(np.float32)
    bq, bv, bf = case.step(q, v, u, nstep, levels=2)
    out = 0.0
    for _ in range(draws):
        up = jit.integers(0, 2, q32.size).astype(bool)
        qj = np.where(up, np.nextafter(q32, np.float32(np.inf)), np.nextafter(q32, np.float32(-np.inf))).astype(np.float64)
        gq, gv, gf = case.step(qj, v, u, nstep, levels=2)
        worst = max([error(gf[k], bf[k]) for k in VECTORS if nstep == 1] + [float(np.abs((gq - qj) - (bq - q)).max()), float(np.abs(gv - bv).max())])
        out = max(out, np.inf if nstep == 1 and gf["nefc"] != bf["nefc"] else worst)
    return out


def sensitivity(name, n, nstep=1):
    """[n]: world_sensitivity of the worlds of a case, as states() recorded it"""
    return np.array([f["sens%d" % nstep] for f in CASES[name].states(n)["figures"]])


def coverage(name, n=N_WORLDS):
    """from the reference alone: which sides of which switches the worlds of a case are on"""
    rows = reference(name, n)
    lim = {}
    for r in rows:
        for kind, ent, side, _, active in r["margins"]["limit"]:
            lim.setdefault((kind, ent), set()).add(("below", "above")[side] if active else "clear-" + ("low", "high")[side])
    pieces = {int(z[2]) for r in rows for z in r["margins"]["zone"]}
    clamps = {}
    for r in rows:
        for what, a, dist, hit in r["margins"]["clamp"]:
            clamps.setdefault((what, a), set()).add("on" if dist == 0.0 else "hit" if hit else "free")
    return dict(limit=lim, pieces=pieces, clamps=clamps, nefc=[r["nefc"] for r in rows])
