"""An fp64 numpy reference for the joint-space constraint rows, the actuators and the integrators, on top of tests/dyn_refs.py (tests/test_cpu_constraint_refs.py holds it to
closed forms; tests/test_cpu_constraint_rows.py and tests/test_gpu_constraint_rows.py compare the compiler, the oracle, the emulator and the device with it).  It imports
nothing of the package or the oracle, reads no MJCF and no compiled table.

Input: the tree of dyn_refs, extended.  Per hinge / slide joint: range (None or (lo, hi)), margin, solreflimit, solimplimit, frictionloss, solreffriction, solimpfriction.
tree["tendons"]: dict(joints [(joint name, coef)], range, margin, solref, solimp) -- fixed, limited.  tree["equalities"]: dict(joint1, joint2, polycoef [5], solref,
solimp, active).  tree["actuators"]: dict(joint, gear, gain, bias [3], ctrlrange (None or (lo, hi)), forcerange).  tree["integrator"]: "Euler" or "RK4".

Constants (MuJoCo's documented mj_setConst): with M at qpos0, dof_invweight0[d] = (M^-1)_dd (a free joint: the mean of its three translational and of its three rotational
entries), tendon_invweight0 = c' M^-1 c, a joint equality's weight = the sum of its two dofs' dof_invweight0.

Rows (MuJoCo's documented constraint model), in the order equalities, friction loss (by dof), joint limits (by joint, lower then upper), tendon limits: Jacobian, residual
pos, margin, impedance d(pos - margin), stiffness and damping from solref, aref = -b (J v) - k d (pos - margin), R = max(MINVAL, (1 - d) / d diagApprox), D = 1 / R.

qacc = argmin_a 1/2 (a - a_s)' M (a - a_s) + sum_i s_i(J_i a - aref_i), s = 1/2 D r^2 (equality), 1/2 D min(0, r)^2 (limit), Huber with linear zone |r| > R f (friction
loss).  solve() guesses each row's piece, solves the linear system of that guess, re-reads the pieces and repeats (where the guesses would cycle it moves only part of the
way, as far as the cost falls); the answer is accepted only by its certificate: the KKT
residual |M (a - a_s) - J' f(a)|_inf and every row's piece consistency to CERT max(1, scale).  No line search, no Newton direction on the cost: nothing of the oracle's or
the engine's algorithm."""
import numpy as np

import dyn_refs as R

MINVAL, MINIMP, MAXIMP = 1e-15, 1e-4, 0.9999
SOLREF, SOLIMP = (0.02, 1.0), (0.9, 0.95, 0.001, 0.5, 2.0)
CERT = 1e-10
EQ, FRICTION, LIMIT, TENDON = "equality", "friction", "limit", "tendon"


def joints(tree):
    """{joint name: (joint dict, qpos address, dof address)}, and the names in order"""
    out, order = {}, []
    for b, k, qa, da in R.layout(tree)[0]:
        j = tree["bodies"][b]["joints"][k]
        out[j["name"]] = (j, qa, da)
        order.append(j["name"])
    return out, order


def mass_matrix(tree, q):
    return R.evaluate(tree, q, np.zeros(R.layout(tree)[2]), levels=1)["M"]


def constants(tree):
    """dict(dof_invweight0 [nv], tendon_invweight0 [ntendon], eq_invweight [neq], Minv0)"""
    jn, _ = joints(tree)
    nv = R.layout(tree)[2]
    Minv = np.linalg.inv(mass_matrix(tree, R.qpos0(tree)))
    w = np.diag(Minv).copy()
    for j, qa, da in jn.values():
        if j["type"] == "free":
            w[da:da + 3], w[da + 3:da + 6] = w[da:da + 3].mean(), w[da + 3:da + 6].mean()
    tw = []
    for t in tree.get("tendons", ()):
        c = tendon_coefs(tree, t, jn)
        tw.append(float(c @ Minv @ c))
    ew = [float(w[jn[e["joint1"]][2]] + w[jn[e["joint2"]][2]]) for e in tree.get("equalities", ())]
    return dict(dof_invweight0=w, tendon_invweight0=np.array(tw), eq_invweight=np.array(ew), nv=nv)


def tendon_coefs(tree, t, jn=None):
    jn = jn or joints(tree)[0]
    c = np.zeros(R.layout(tree)[2])
    for name, coef in t["joints"]:
        c[jn[name][2]] += coef      # a joint listed twice counts twice
    return c


def tendon_length(tree, t, q, jn=None):
    jn = jn or joints(tree)[0]
    return float(sum(coef * q[jn[name][1]] for name, coef in t["joints"]))


def impedance(solimp, x):
    """the five-value solimp curve d(|x|) with its clamps"""
    d0, d1 = (min(MAXIMP, max(MINIMP, s)) for s in solimp[:2])
    width, mid, power = max(0.0, solimp[2]), min(MAXIMP, max(MINIMP, solimp[3])), max(1.0, solimp[4])
    if d0 == d1 or width <= MINVAL:
        return 0.5 * (d0 + d1)
    x = abs(x) / width
    if x >= 1.0:
        return d1
    if x <= 0.0:
        return d0
    y = x ** power / mid ** (power - 1.0) if x <= mid else 1.0 - (1.0 - x) ** power / (1.0 - mid) ** (power - 1.0)
    return d0 + y * (d1 - d0)


def stiffness_damping(solref, solimp, h):
    dmax = min(MAXIMP, max(MINIMP, solimp[1]))
    if solref[0] > 0:
        tc, dr = max(solref[0], 2.0 * h), solref[1]      # refsafe: a time constant below two timesteps is raised to them
        return 1.0 / (dmax * dmax * tc * tc * dr * dr), 2.0 / (dmax * tc)
    return -solref[0] / (dmax * dmax), -solref[1] / dmax


def actuation(tree, q, v, ctrl):
    """dict(qfrc_actuator [nv], force [nu] (clamped), margins [(what, actuator, distance from the clamp)])"""
    jn, _ = joints(tree)
    out, forces, margins = np.zeros(R.layout(tree)[2]), [], []
    for a, act in enumerate(tree.get("actuators", ())):
        j, qa, da = jn[act["joint"]]
        u, g = float(ctrl[a]), act["gear"]
        if act.get("ctrlrange") is not None:
            lo, hi = act["ctrlrange"]
            margins.append(("ctrl", a, min(abs(u - lo), abs(u - hi)), u < lo or u > hi))
            u = min(hi, max(lo, u))
        f = act["gain"] * u + act["bias"][0] + act["bias"][1] * (g * q[qa]) + act["bias"][2] * (g * v[da])
        if act.get("forcerange") is not None:
            lo, hi = act["forcerange"]
            margins.append(("force", a, min(abs(f - lo), abs(f - hi)), f < lo or f > hi))
            f = min(hi, max(lo, f))
        forces.append(f)
        out[da] += g * f      # the forces of two actuators on one joint add
    return dict(qfrc_actuator=out, force=np.array(forces), margins=margins)


def rows(tree, q, v, consts=None):
    """the constraint rows of the state: dict(kind [n], id [n] (entity, side), J [n, nv], pos, margin, aref, D, R, floss, imp [n]) and margins: per limit side of every
    limited joint and tendon |dist - margin| (what, entity, side, value, active)"""
    consts = consts or constants(tree)
    jn, order = joints(tree)
    nv, h = R.layout(tree)[2], float(tree["timestep"])
    kind, ids, J, pos, mg, prm, floss, switch = [], [], [], [], [], [], [], []

    def add(k, i, row, p, m, solref, solimp, diag, f=0.0):
        kind.append(k), ids.append(i), J.append(row), pos.append(p), mg.append(m), prm.append((solref, solimp, diag)), floss.append(f)

    e_ = lambda d: np.eye(nv)[d]
    for n, e in enumerate(tree.get("equalities", ())):
        if not e.get("active", True):
            continue
        (j1, q1, d1), (j2, q2, d2) = jn[e["joint1"]], jn[e["joint2"]]
        c, x = e["polycoef"], q[q2] - R.qpos0(tree)[q2]
        poly = c[0] + c[1] * x + c[2] * x ** 2 + c[3] * x ** 3 + c[4] * x ** 4
        dpoly = c[1] + 2.0 * c[2] * x + 3.0 * c[3] * x ** 2 + 4.0 * c[4] * x ** 3
        add(EQ, (n, 0), e_(d1) - dpoly * e_(d2), (q[q1] - R.qpos0(tree)[q1]) - poly, 0.0, e.get("solref", SOLREF), e.get("solimp", SOLIMP), consts["eq_invweight"][n])
    for name in order:
        j, qa, da = jn[name]
        if j["type"] != "free" and j.get("frictionloss", 0.0) > 0:
            add(FRICTION, (da, 0), e_(da), 0.0, 0.0, j.get("solreffriction", SOLREF), j.get("solimpfriction", SOLIMP), consts["dof_invweight0"][da], j["frictionloss"])
    for n, name in enumerate(order):
        j, qa, da = jn[name]
        if j["type"] == "free" or j.get("range") is None:
            continue
        m = j.get("margin", 0.0)
        for side, (dist, sign) in enumerate(((q[qa] - j["range"][0], 1.0), (j["range"][1] - q[qa], -1.0))):
            switch.append((LIMIT, n, side, abs(dist - m), dist < m))
            if dist < m:
                add(LIMIT, (n, side), sign * e_(da), dist, m, j.get("solreflimit", SOLREF), j.get("solimplimit", SOLIMP), consts["dof_invweight0"][da])
    for n, t in enumerate(tree.get("tendons", ())):
        c, ln, m = tendon_coefs(tree, t, jn), tendon_length(tree, t, q, jn), t.get("margin", 0.0)
        for side, (dist, sign) in enumerate(((ln - t["range"][0], 1.0), (t["range"][1] - ln, -1.0))):
            switch.append((TENDON, n, side, abs(dist - m), dist < m))
            if dist < m:
                add(TENDON, (n, side), sign * c, dist, m, t.get("solref", SOLREF), t.get("solimp", SOLIMP), consts["tendon_invweight0"][n])
    n = len(kind)
    J = np.array(J).reshape(n, nv)
    pos, mg, floss = np.array(pos), np.array(mg), np.array(floss)
    aref, D, Rr, imp = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for r in range(n):
        solref, solimp, diag = prm[r]
        imp[r] = impedance(solimp, pos[r] - mg[r])
        k, b = stiffness_damping(solref, solimp, h)
        if kind[r] == FRICTION:
            k = 0.0
        Rr[r] = max(MINVAL, (1.0 - imp[r]) / imp[r] * diag)
        D[r] = 1.0 / Rr[r]
        aref[r] = -b * (J[r] @ v) - k * imp[r] * (pos[r] - mg[r])
    return dict(kind=kind, id=ids, J=J, pos=pos, margin=mg, aref=aref, D=D, R=Rr, floss=floss, imp=imp, switch=switch)


def row_forces(rw, a):
    """(force [n], piece [n]) of the rows at the acceleration a: piece 0 quadratic, -1 / +1 the linear zones of a friction row (r below -R f / above R f), 2 an inactive limit"""
    r = rw["J"] @ a - rw["aref"]
    f, piece = np.zeros(len(r)), np.zeros(len(r), dtype=int)
    for i, k in enumerate(rw["kind"]):
        if k == EQ:
            f[i] = -rw["D"][i] * r[i]
        elif k == FRICTION:
            z = rw["R"][i] * rw["floss"][i]
            piece[i] = -1 if r[i] < -z else 1 if r[i] > z else 0
            f[i] = rw["floss"][i] if piece[i] < 0 else -rw["floss"][i] if piece[i] > 0 else -rw["D"][i] * r[i]
        else:
            piece[i] = 0 if r[i] < 0 else 2
            f[i] = -rw["D"][i] * min(0.0, r[i])
    return f, piece


def solve(M, a_s, rw, max_iter=200):
    """dict(qacc, force, piece, kkt, scale, iterations, zone [per friction row ||r| - R f| / (R f)]): the minimiser by active-set fixed point, accepted by its certificate"""
    n, nv = len(rw["kind"]), len(a_s)
    if not n:
        return dict(qacc=np.array(a_s, dtype=np.float64), force=np.zeros(0), piece=np.zeros(0, dtype=int), kkt=0.0, scale=1.0, iterations=0, zone=[])
    J, D, aref, fl = rw["J"], rw["D"], rw["aref"], rw["floss"]
    _, piece = row_forces(rw, a_s)
    kinds, z = np.array(rw["kind"]), rw["R"] * fl

    def cost(x):
        r = J @ x - aref
        s = np.where(kinds == EQ, 0.5 * D * r * r, np.where(kinds == FRICTION, np.where(np.abs(r) <= z, 0.5 * D * r * r, fl * (np.abs(r) - 0.5 * z)), 0.5 * D * np.minimum(0.0, r) ** 2))
        return 0.5 * (x - a_s) @ M @ (x - a_s) + s.sum()

    a = np.array(a_s, dtype=np.float64)
    for it in range(max_iter):
        quad = piece == 0
        lin = np.where(piece == -1, fl, np.where(piece == 1, -fl, 0.0))
        A = M + J[quad].T @ (D[quad, None] * J[quad])
        new_a = np.linalg.solve(A, M @ a_s + J[quad].T @ (D[quad] * aref[quad]) + J.T @ lin)
        _, new = row_forces(rw, new_a)
        if np.array_equal(new, piece):
            a = new_a
            break
        # the guess was wrong: move towards its answer, the whole way if the cost falls, else half of it, a quarter ... (the guesses of a full move can cycle), and re-read
        t, c0 = 1.0, cost(a)
        while t > 1e-12 and not cost(a + t * (new_a - a)) < c0:
            t *= 0.5
        a = a + t * (new_a - a)
        _, piece = row_forces(rw, a)
    else:
        raise RuntimeError("the active-set iteration did not settle")
    f, again = row_forces(rw, a)
    assert np.array_equal(again, piece)
    lhs, rhs = M @ (a - a_s), J.T @ f
    scale = max(1.0, float(np.abs(M @ a_s).max()), float(np.abs(rhs).max()))
    kkt = float(np.abs(lhs - rhs).max())
    r = J @ a - aref
    zone = [(i, abs(abs(r[i]) - rw["R"][i] * fl[i]) / (rw["R"][i] * fl[i]), int(piece[i])) for i in range(n) if rw["kind"][i] == FRICTION]
    if not kkt <= CERT * scale:
        raise RuntimeError(f"no certificate: KKT residual {kkt:.3e}, scale {scale:.3e}")
    return dict(qacc=a, force=f, piece=piece, kkt=kkt, scale=scale, iterations=it + 1, zone=zone)


def forward(tree, q, v, ctrl=None, consts=None, levels=R.LEVELS):
    """one forward pass: the fields of dyn_refs.evaluate with the actuators in qfrc_smooth, plus qfrc_actuator, the rows (efc_*), qfrc_constraint, qacc, the certificate and
    the switch margins"""
    q, v = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)
    nu = len(tree.get("actuators", ()))
    ctrl = np.zeros(nu) if ctrl is None else np.asarray(ctrl, dtype=np.float64)
    out = R.evaluate(tree, q, v, levels=levels)
    act = actuation(tree, q, v, ctrl)
    M = out["M"]
    smooth = out["qfrc_smooth"] + act["qfrc_actuator"]
    a_s = np.linalg.solve(M, smooth)
    rw = rows(tree, q, v, consts)
    sol = solve(M, a_s, rw)
    fc = rw["J"].T @ sol["force"] if len(rw["kind"]) else np.zeros(len(v))
    out.update(qfrc_actuator=act["qfrc_actuator"], act_force=act["force"], qfrc_smooth=smooth, qacc_smooth=a_s, qacc=sol["qacc"], qfrc_constraint=fc, nefc=len(rw["kind"]),
               efc_kind=rw["kind"], efc_id=rw["id"], efc_J=rw["J"], efc_pos=rw["pos"], efc_margin=rw["margin"], efc_aref=rw["aref"], efc_D=rw["D"], efc_R=rw["R"],
               efc_floss=rw["floss"], efc_force=sol["force"], efc_piece=sol["piece"], kkt=sol["kkt"], kkt_scale=sol["scale"], iterations=sol["iterations"],
               margins=dict(limit=rw["switch"], zone=sol["zone"], clamp=act["margins"]))
    return out


def step(tree, q, v, ctrl=None, nstep=1, consts=None, levels=R.LEVELS):
    """(qpos, qvel, the forward pass at the start of the last step) after nstep steps of the tree's integrator"""
    q, v = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)
    consts = consts or constants(tree)
    h = float(tree["timestep"])
    fwd = None
    for _ in range(nstep):
        if tree.get("integrator", "Euler") == "RK4":      # the classical tableau over four full forward passes; no implicit damping
            X, F = (q, v), []
            for stage, c in enumerate((0.5, 0.5, 1.0, None)):
                f = forward(tree, X[0], X[1], ctrl, consts, levels)
                fwd = f if stage == 0 else fwd
                F.append((X[1], f["qacc"]))
                if c is not None:
                    X = (R.integrate_pos(tree, q, F[-1][0], c * h), v + c * h * F[-1][1])
            dv = (F[0][0] + 2.0 * F[1][0] + 2.0 * F[2][0] + F[3][0]) / 6.0
            da = (F[0][1] + 2.0 * F[1][1] + 2.0 * F[2][1] + F[3][1]) / 6.0
            q, v = R.integrate_pos(tree, q, dv, h), v + h * da
        else:      # semi-implicit Euler: the constraint force on the right of dyn_refs's implicit-damping system
            fwd = forward(tree, q, v, ctrl, consts, levels)
            _, damp = R._dof_params(tree)
            v = v + h * np.linalg.solve(fwd["M"] + h * np.diag(damp), fwd["qfrc_smooth"] + fwd["qfrc_constraint"])
            q = R.integrate_pos(tree, q, v, h)
    return q, v, fwd
