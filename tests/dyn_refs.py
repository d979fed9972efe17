"""An fp64 numpy reference for kinematics and smooth dynamics of a kinematic tree, written from the definitions (tests/test_cpu_dyn_refs.py holds it to closed forms;
tests/test_cpu_dyn_trees.py and tests/test_gpu_dyn_trees.py compare the compiler, the oracle, the emulator and the device with it).  It imports nothing of the package or the
oracle, reads no MJCF and no compiled table, and shares no formula with them: no cdof, no composite inertias, no recursive Newton-Euler.

Input: a tree, dict(gravity [3], timestep, bodies [...]).  bodies[k] = dict(name, parent (index into bodies, -1: the world; parents come first), pos [3], quat [4] (pose in the
parent at qpos = ref), joints (ordered; dict(type "free" / "hinge" / "slide", pos [3] (anchor, body frame), axis [3] (unit, body frame), ref, armature, damping, stiffness,
springref)), mass, ipos [3], inertia [3, 3] (about ipos, body frame), sites (dict(name, pos, quat))).  qpos / qvel are laid out body by body, joint by joint.

Joint semantics (MuJoCo's documentation): the written pose of a body is its pose at qpos = ref; the joints of one body apply in order, each in the frame the ones before it
left; a hinge turns everything after it about its axis through its anchor by q - ref; a slide moves it along its axis by q - ref; a free joint's qpos IS the world pose
(position, unit quaternion), its linear velocity is in the world frame and its angular velocity in the body's own frame.

Forces.  M = sum_b m Jp' Jp + Jr' (R I R') Jr + diag(armature) with the geometric Jacobians of the centres of mass; qfrc_bias = sum_b Jp' m (a_b - g) + Jr' (I_w alpha_b +
omega_b x I_w omega_b), where a_b and alpha_b are the time derivatives of Jp_b v and Jr_b v along the constant-qvel trajectory integrate_pos(q, v, t): central differences with
Richardson extrapolation, whose last correction (plus the change under a second set of steps) is the reference's own error estimate (`err`)."""
import numpy as np

U = 2.0 ** -52
H0, LEVELS = 2e-3, 4      # first difference step [s] and Richardson levels: error O((H0 |omega|)^8); tests/test_cpu_dyn_refs.py checks the estimates of every case


def qmul(p, q):
    return np.array([p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                     p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]])


def qmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def qexp(theta):
    """the unit quaternion of the rotation vector theta"""
    a = np.linalg.norm(theta)
    if a < 1e-300:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.r_[np.cos(a / 2), np.sin(a / 2) * np.asarray(theta) / a]


def unit(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def sign_like(q, ref):
    """quaternions are compared up to sign: q with the sign that brings it nearer to ref"""
    s = np.sign((np.asarray(q) * np.asarray(ref)).sum(axis=-1, keepdims=True))
    return np.where(s == 0, 1.0, s) * np.asarray(q)


def layout(tree):
    """per joint (body, joint index in body, qpos address, dof address), nq, nv"""
    out, nq, nv = [], 0, 0
    for b, body in enumerate(tree["bodies"]):
        for k, j in enumerate(body["joints"]):
            out.append((b, k, nq, nv))
            nq, nv = nq + (7 if j["type"] == "free" else 1), nv + (6 if j["type"] == "free" else 1)
    return out, nq, nv


def qpos0(tree):
    lay, nq, _ = layout(tree)
    q = np.zeros(nq)
    kin = None
    for b, k, qa, _ in lay:
        j = tree["bodies"][b]["joints"][k]
        if j["type"] == "free":
            if kin is None:
                kin = _rest_poses(tree)
            q[qa:qa + 3], q[qa + 3:qa + 7] = kin[0][b], kin[1][b]
        else:
            q[qa] = j["ref"]
    return q


def _rest_poses(tree):
    pos, quat = [], []
    for body in tree["bodies"]:
        p = body["parent"]
        pp, pq = (np.zeros(3), np.array([1.0, 0, 0, 0])) if p < 0 else (pos[p], quat[p])
        pos.append(pp + qmat(pq) @ np.asarray(body["pos"], dtype=np.float64))
        quat.append(unit(qmul(pq, unit(body["quat"]))))
    return pos, quat


def integrate_pos(tree, q, v, t):
    """the configuration reached from q after moving with the constant velocity v for the time t"""
    lay, nq, _ = layout(tree)
    out = np.array(q, dtype=np.float64)
    for b, k, qa, da in lay:
        if tree["bodies"][b]["joints"][k]["type"] == "free":
            out[qa:qa + 3] = q[qa:qa + 3] + t * v[da:da + 3]
            out[qa + 3:qa + 7] = unit(qmul(unit(q[qa + 3:qa + 7]), qexp(t * np.asarray(v[da + 3:da + 6]))))
        else:
            out[qa] = q[qa] + t * v[da]
    return out


def kinematics(tree, q):
    """dict(xpos [nb, 3], xquat [nb, 4], xmat [nb, 3, 3], xipos [nb, 3], site_xpos / site_xmat / site_body, and per dof its world axis, world anchor, kind (0: translation
    along the axis, 1: rotation about the axis through the anchor) and body)"""
    bodies = tree["bodies"]
    lay, nq, nv = layout(tree)
    adr = {(b, k): (qa, da) for b, k, qa, da in lay}
    nb = len(bodies)
    xpos, xquat, xmat, xipos = np.zeros((nb, 3)), np.zeros((nb, 4)), np.zeros((nb, 3, 3)), np.zeros((nb, 3))
    axis, anchor, kind, dbody = np.zeros((nv, 3)), np.zeros((nv, 3)), np.zeros(nv, dtype=int), np.zeros(nv, dtype=int)
    sp, sm, sb, sn = [], [], [], []
    for b, body in enumerate(bodies):
        p = body["parent"]
        pp, pq = (np.zeros(3), np.array([1.0, 0, 0, 0])) if p < 0 else (xpos[p], xquat[p])
        pos, quat = pp + qmat(pq) @ np.asarray(body["pos"], dtype=np.float64), unit(qmul(pq, unit(body["quat"])))
        for k, j in enumerate(body["joints"]):
            qa, da = adr[(b, k)]
            if j["type"] == "free":
                pos, quat = np.array(q[qa:qa + 3], dtype=np.float64), unit(q[qa + 3:qa + 7])
                R = qmat(quat)
                axis[da:da + 3], kind[da:da + 3] = np.eye(3), 0
                axis[da + 3:da + 6], anchor[da + 3:da + 6], kind[da + 3:da + 6] = R.T, pos, 1
                dbody[da:da + 6] = b
                continue
            R = qmat(quat)
            ax, jp = np.asarray(j["axis"], dtype=np.float64), np.asarray(j["pos"], dtype=np.float64)
            axis[da], anchor[da], dbody[da] = R @ ax, pos + R @ jp, b
            d = q[qa] - j["ref"]
            if j["type"] == "slide":
                kind[da] = 0
                pos = pos + d * axis[da]
            else:
                kind[da] = 1
                quat = unit(qmul(quat, qexp(d * ax)))
                pos = anchor[da] - qmat(quat) @ jp      # the anchor stays where it is
        xpos[b], xquat[b], xmat[b] = pos, quat, qmat(quat)
        xipos[b] = pos + xmat[b] @ np.asarray(body["ipos"], dtype=np.float64)
        for s in body.get("sites", ()):
            sp.append(pos + xmat[b] @ np.asarray(s["pos"], dtype=np.float64))
            sm.append(xmat[b] @ qmat(unit(s["quat"])))
            sb.append(b)
            sn.append(s["name"])
    return dict(xpos=xpos, xquat=xquat, xmat=xmat, xipos=xipos, site_xpos=np.array(sp).reshape(-1, 3), site_xmat=np.array(sm).reshape(-1, 3, 3), site_body=np.array(sb, dtype=int),
                site_names=sn, axis=axis, anchor=anchor, kind=kind, dof_body=dbody)


def ancestors(tree):
    """[nb, nb] bool: A[b, a] -- a is b or one of its ancestors"""
    nb = len(tree["bodies"])
    A = np.eye(nb, dtype=bool)
    for b, body in enumerate(tree["bodies"]):
        if body["parent"] >= 0:
            A[b] |= A[body["parent"]]
    return A


def jacobians(tree, kin, points, point_body):
    """(jacp, jacr) [n, 3, nv] of world points fixed to the bodies point_body: a dof moves a point when its body is the point's body or an ancestor of it; a translation
    moves it along the axis, a rotation by axis x (point - anchor)"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    moves = ancestors(tree)[np.asarray(point_body, dtype=int)][:, kin["dof_body"]]      # [n, nv]
    rot = kin["kind"] == 1
    arm = points[:, None, :] - kin["anchor"][None]
    jp = np.where(rot[None, :, None], np.cross(kin["axis"][None], arm), kin["axis"][None])
    jr = np.where(rot[None, :, None], kin["axis"][None], 0.0) + np.zeros_like(jp)
    jp, jr = jp * moves[:, :, None], jr * moves[:, :, None]
    return np.ascontiguousarray(jp.transpose(0, 2, 1)), np.ascontiguousarray(jr.transpose(0, 2, 1))


def _dof_params(tree):
    _, nq, nv = layout(tree)
    arm, damp = np.zeros(nv), np.zeros(nv)
    for b, k, qa, da in layout(tree)[0]:
        j = tree["bodies"][b]["joints"][k]
        n = 6 if j["type"] == "free" else 1
        arm[da:da + n], damp[da:da + n] = j.get("armature", 0.0), j.get("damping", 0.0)
    return arm, damp


def _body_velocities(tree, q, v):
    """centre-of-mass velocities and angular velocities of all bodies, stacked [2, nb, 3]"""
    kin = kinematics(tree, q)
    jp, jr = jacobians(tree, kin, kin["xipos"], np.arange(len(tree["bodies"])))
    return np.stack([jp @ v, jr @ v])


def _accelerations(tree, q, v, levels, h0):
    """d/dt of _body_velocities along integrate_pos(q, v, t) at t = 0: the Richardson tableau's last entry and its last correction"""
    D = lambda h: (_body_velocities(tree, integrate_pos(tree, q, v, h), v) - _body_velocities(tree, integrate_pos(tree, q, v, -h), v)) / (2.0 * h)
    row = [D(h0 / 2 ** k) for k in range(levels)]
    prev = row[-1]
    for n in range(1, levels):
        prev = row[-1]
        row = [(4.0 ** n * row[k + 1] - row[k]) / (4.0 ** n - 1.0) for k in range(len(row) - 1)]
    return row[0], row[0] - prev


def _acceleration_estimate(tree, q, v, levels, h0):
    """(value, error estimate): the estimate is the last Richardson correction -- what is left of the truncation -- plus the change of the answer when every step is made
    3/4 as long, which also sees the rounding noise of the differences (u |velocity| / step), something the correction alone need not"""
    acc, corr = _accelerations(tree, q, v, levels, h0)
    if levels < 2:
        return acc, np.abs(corr)
    alt, _ = _accelerations(tree, q, v, levels, 0.75 * h0)
    return acc, np.abs(corr) + np.abs(acc - alt)


def evaluate(tree, q, v, levels=LEVELS, h0=H0):
    """everything the comparisons read, for one world: dict of fields, plus out["err"]: per field the reference's own error estimate (same shape or scalar)"""
    bodies = tree["bodies"]
    nb = len(bodies)
    lay, nq, nv = layout(tree)
    q, v = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)
    g, h = np.asarray(tree["gravity"], dtype=np.float64), float(tree["timestep"])
    kin = kinematics(tree, q)
    jp, jr = jacobians(tree, kin, kin["xipos"], np.arange(nb))
    arm, damp = _dof_params(tree)
    mass = np.array([b["mass"] for b in bodies], dtype=np.float64)
    Iw = np.stack([kin["xmat"][b] @ np.asarray(bodies[b]["inertia"], dtype=np.float64) @ kin["xmat"][b].T for b in range(nb)])
    M = np.einsum("b,bki,bkj->ij", mass, jp, jp) + np.einsum("bki,bkl,blj->ij", jr, Iw, jr) + np.diag(arm)
    vel = np.stack([jp @ v, jr @ v])
    acc, acc_err = _acceleration_estimate(tree, q, v, levels, h0)
    gyro = np.cross(vel[1], np.einsum("bkl,bl->bk", Iw, vel[1]))

    def bias_of(a):
        return np.einsum("bki,bk->i", jp, mass[:, None] * (a[0] - g)) + np.einsum("bki,bk->i", jr, np.einsum("bkl,bl->bk", Iw, a[1]) + gyro)

    bias = bias_of(acc)
    bias_err = np.einsum("bki,bk->i", np.abs(jp), mass[:, None] * acc_err[0]) + np.einsum("bki,bk->i", np.abs(jr), np.einsum("bkl,bl->bk", np.abs(Iw), acc_err[1]))
    passive = np.zeros(nv)
    for b, k, qa, da in lay:
        j = bodies[b]["joints"][k]
        if j["type"] != "free":
            passive[da] = -j.get("damping", 0.0) * v[da] - j.get("stiffness", 0.0) * (q[qa] - j.get("springref", 0.0))
    smooth = passive - bias
    qacc = np.linalg.solve(M, smooth) if nv else np.zeros(0)
    Mh = M + h * np.diag(damp)
    qacc_euler = np.linalg.solve(Mh, smooth) if nv else np.zeros(0)
    v1 = v + h * qacc_euler
    q1 = integrate_pos(tree, q, v1, h)
    sjp, sjr = jacobians(tree, kin, kin["site_xpos"], kin["site_body"])
    out = dict(xpos=kin["xpos"], xquat=kin["xquat"], xmat=kin["xmat"], xipos=kin["xipos"], site_xpos=kin["site_xpos"], site_xmat=kin["site_xmat"], site_jacp=sjp, site_jacr=sjr,
               site_xvelp=sjp @ v, site_xvelr=sjr @ v, M=M, qfrc_bias=bias, qfrc_passive=passive, qfrc_smooth=smooth, qacc_smooth=qacc, qacc=qacc.copy(), qvel1=v1, qpos1=q1,
               com_jacp=jp, com_jacr=jr, com_vel=vel, Iw=Iw, site_names=kin["site_names"], body_names=[b["name"] for b in bodies])
    # the reference's own error.  Rounding: each level of the tree is a quaternion product, a rotation and a sum, some 32 roundings relative to the field's scale, so eps =
    # 32 u depth relative for everything formed from the poses (a sum of nb terms of one sign adds nb u, which is nothing next to it).  The differences: bias_err, carried
    # through.  A solve M a = b with |dM| <= eps |M| and |db| <= eps |b| + bias_err moves a by at most |M^-1| (eps (|M| |a| + |b|) + bias_err), componentwise.
    depth = int(ancestors(tree).sum(axis=1).max()) if nb else 1
    eps = 32.0 * U * depth
    scale = lambda k: max(1.0, float(np.abs(out[k]).max())) if np.asarray(out[k]).size else 1.0
    solve_err = lambda A, x: np.abs(np.linalg.inv(A)) @ (eps * (np.abs(A) @ np.abs(x) + np.abs(smooth)) + bias_err) if nv else np.zeros(0)
    err = {k: eps * scale(k) for k in ("xpos", "xquat", "xmat", "xipos", "site_xpos", "site_xmat", "site_jacp", "site_jacr", "site_xvelp", "site_xvelr", "qfrc_passive", "M")}
    err["qfrc_bias"] = bias_err + eps * scale("qfrc_bias")
    err["qfrc_smooth"] = bias_err + eps * scale("qfrc_smooth")
    err["qacc_smooth"] = solve_err(M, qacc)
    err["qacc"] = err["qacc_smooth"]
    err["qvel1"] = eps * scale("qvel1") + h * solve_err(Mh, qacc_euler)
    err["qpos1"] = np.full(nq, eps * scale("qpos1") + h * float(np.max(err["qvel1"], initial=0.0)))
    err["richardson"] = dict(acc=float(np.abs(acc_err).max(initial=0.0)), acc_scale=float(np.abs(acc).max(initial=0.0)), qfrc_bias=float(bias_err.max(initial=0.0)))
    out["err"] = err
    return out
