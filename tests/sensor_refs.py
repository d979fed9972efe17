"""An fp64 numpy reference for the sensor readings of BatchedSim (gymnasium_robotics_amd/sim.py, SENSORS), written from the definitions on top of tests/dyn_refs.py
(kinematics, jacobians, integrate_pos, evaluate): no cdof, no spatial algebra, nothing of the engine.  tests/test_cpu_sensor_refs.py holds it to closed forms.

A sensor is dict(name, type, objtype ("site" / "xbody" / "joint"), objname, cutoff).  For an object with position p, rotation R (local -> world) and Jacobians Jp, Jr of the
material point p:   u = Jp v,   omega = Jr v,   c = Jp a + (d/dt Jp) v,   alpha = Jr a + (d/dt Jr) v,   a = qacc of the pass (dyn_refs.evaluate: the trees have no contacts).
(d/dt J) v is the time derivative of J(q(t)) v along the constant-qvel trajectory integrate_pos(q, v, t), the material point moving with its body: central differences with
Richardson extrapolation, the scheme and the error estimate of dyn_refs (H0, LEVELS)."""
import numpy as np

import dyn_refs as R

DIM = dict(jointpos=1, jointvel=1, framepos=3, framequat=4, framexaxis=3, frameyaxis=3, framezaxis=3, framelinvel=3, frameangvel=3, velocimeter=3, gyro=3, framelinacc=3,
           frameangacc=3, accelerometer=3)
POSITION = ("framepos", "framequat", "framexaxis", "frameyaxis", "framezaxis")
VELOCITY = ("framelinvel", "frameangvel", "velocimeter", "gyro")
JOINT = ("jointpos", "jointvel")
ACCELERATION = ("framelinacc", "frameangacc", "accelerometer")
NO_CUTOFF = ("framequat", "framexaxis", "frameyaxis", "framezaxis")


def mat2quat(M):
    """the unit quaternion (w >= 0) of a rotation matrix, from the eigenvector of the symmetric 4 x 4 form (no branch on the trace)"""
    K = np.array([[M[0, 0] - M[1, 1] - M[2, 2], 0, 0, 0], [M[0, 1] + M[1, 0], M[1, 1] - M[0, 0] - M[2, 2], 0, 0], [M[0, 2] + M[2, 0], M[1, 2] + M[2, 1], M[2, 2] - M[0, 0] - M[1, 1], 0],
                  [M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1], M[0, 0] + M[1, 1] + M[2, 2]]]) / 3.0
    w, V = np.linalg.eigh(K)
    q = V[[3, 0, 1, 2], np.argmax(w)]
    return q if q[0] >= 0 else -q


def layout(sensors):
    """{name: (adr, dim)} and ndata, in the order given"""
    out, adr = {}, 0
    for s in sensors:
        out[s["name"]] = (adr, DIM[s["type"]])
        adr += DIM[s["type"]]
    return out, adr


def _objects(tree, kin, sensors):
    """per frame sensor: (point [3], rotation [3, 3], body)"""
    names = [b["name"] for b in tree["bodies"]]
    out = {}
    for s in sensors:
        if s["type"] in JOINT:
            continue
        if s["objtype"] == "site":
            k = kin["site_names"].index(s["objname"])
            out[s["name"]] = (kin["site_xpos"][k], kin["site_xmat"][k], int(kin["site_body"][k]))
        else:
            b = names.index(s["objname"])
            out[s["name"]] = (kin["xpos"][b], kin["xmat"][b], b)
    return out


def _point_velocities(tree, q, v, sensors):
    """[2, n, 3]: u and omega of every frame sensor's material point at the configuration q, moving with v"""
    kin = R.kinematics(tree, q)
    obj = _objects(tree, kin, sensors)
    keys = [s["name"] for s in sensors if s["name"] in obj]
    if not keys:
        return np.zeros((2, 0, 3))
    jp, jr = R.jacobians(tree, kin, np.array([obj[k][0] for k in keys]), np.array([obj[k][2] for k in keys]))
    return np.stack([jp @ v, jr @ v])


def _djv(tree, q, v, sensors, levels, h0):
    D = lambda h: (_point_velocities(tree, R.integrate_pos(tree, q, v, h), v, sensors) - _point_velocities(tree, R.integrate_pos(tree, q, v, -h), v, sensors)) / (2.0 * h)
    row = [D(h0 / 2 ** k) for k in range(levels)]
    prev = row[-1]
    for n in range(1, levels):
        prev = row[-1]
        row = [(4.0 ** n * row[k + 1] - row[k]) / (4.0 ** n - 1.0) for k in range(len(row) - 1)]
    return row[0], row[0] - prev


def djv(tree, q, v, sensors, levels=R.LEVELS, h0=R.H0):
    """((d/dt Jp) v, (d/dt Jr) v) stacked [2, n, 3] for the frame sensors in order, and the error estimate of dyn_refs: the last Richardson correction plus the change under
    steps 3/4 as long"""
    val, corr = _djv(tree, q, v, sensors, levels, h0)
    alt, _ = _djv(tree, q, v, sensors, levels, 0.75 * h0)
    return val, np.abs(corr) + np.abs(val - alt)


def evaluate(tree, q, v, sensors, qacc=None, gravity=None):
    """dict(data [ndata], err [ndata] (the reference's own error estimate), adr {name: (adr, dim)}, qacc).  qacc: the pass's acceleration (default: dyn_refs.evaluate's);
    gravity: default the tree's"""
    q, v = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)
    g = np.asarray(tree["gravity"] if gravity is None else gravity, dtype=np.float64)
    adr, ndata = layout(sensors)
    data, err = np.zeros(ndata), np.zeros(ndata)
    qacc_err = 0.0
    if qacc is None:
        ev = R.evaluate(tree, q, v)
        qacc, qacc_err = ev["qacc"], np.asarray(ev["err"]["qacc"])
    qacc = np.asarray(qacc, dtype=np.float64)
    kin = R.kinematics(tree, q)
    obj = _objects(tree, kin, sensors)
    frames = [s for s in sensors if s["name"] in obj]
    dj, dj_err = djv(tree, q, v, sensors) if frames else (np.zeros((2, 0, 3)), np.zeros((2, 0, 3)))
    jadr = {}
    for b, k, qa, da in R.layout(tree)[0]:
        jadr[tree["bodies"][b]["joints"][k].get("name")] = (qa, da)
    depth = int(R.ancestors(tree).sum(axis=1).max())
    eps = 32.0 * R.U * depth
    for s in sensors:
        a, dim = adr[s["name"]]
        t = s["type"]
        if t in JOINT:
            qa, da = jadr[s["objname"]]
            val, e = np.array([q[qa] if t == "jointpos" else v[da]]), np.zeros(1)
        else:
            p, Rm, b = obj[s["name"]]
            k = [f["name"] for f in frames].index(s["name"])
            jp, jr = R.jacobians(tree, kin, p[None], [b])
            jp, jr = jp[0], jr[0]
            if t == "framepos":
                val = p
            elif t == "framequat":
                val = mat2quat(Rm)
            elif t in ("framexaxis", "frameyaxis", "framezaxis"):
                val = Rm[:, "xyz".index(t[5])]
            elif t == "framelinvel":
                val = jp @ v
            elif t == "frameangvel":
                val = jr @ v
            elif t == "velocimeter":
                val = Rm.T @ (jp @ v)
            elif t == "gyro":
                val = Rm.T @ (jr @ v)
            elif t == "frameangacc":
                val = jr @ qacc + dj[1, k]
            elif t == "framelinacc":
                val = jp @ qacc + dj[0, k] - g
            elif t == "accelerometer":
                val = Rm.T @ (jp @ qacc + dj[0, k] - g)
            else:
                raise KeyError(t)
            e = np.full(dim, eps * max(1.0, float(np.abs(val).max())))
            if t in ACCELERATION:
                J = jr if t == "frameangacc" else jp
                e = e + float((np.abs(J) @ np.broadcast_to(qacc_err, qacc.shape)).max()) + float(dj_err[1 if t == "frameangacc" else 0, k].max()) * (np.sqrt(3.0) if t == "accelerometer" else 1.0)
        cut = float(s.get("cutoff", 0.0))
        if cut > 0 and t not in NO_CUTOFF:
            val = np.clip(val, -cut, cut)
        data[a:a + dim], err[a:a + dim] = val, e
    return dict(data=data, err=err, adr=adr, qacc=qacc)
