"""tests/sensor_refs.py, the fp64 reference of the sensor readings, held to closed forms: a free body with a body-frame angular velocity and a world velocity, the same body in
free fall, and a turntable at a constant rate.  Its own error estimate stays within 1e-8 max(1, |value|), the figure tests/dyn_refs.py is held to."""
import numpy as np

import dyn_refs as R
import sensor_refs as SR

G = np.array([0.4, -0.7, -9.5])
QS = R.unit([0.7, -0.2, 0.5, 0.4])      # the site's frame in the body
RS = np.array([0.07, 0.11, 0.05])      # the site in the body frame: a lever arm of a decimetre, well off the direction of the angular velocity below
SENSORS = [dict(name=t, type=t, objtype="site", objname="imu", cutoff=0.0) for t in ("gyro", "velocimeter", "accelerometer", "framelinacc", "frameangacc", "framequat", "framepos")]


def _free_body(gravity, inertia=(0.004, 0.009, 0.012)):
    free = dict(type="free", name="root", pos=np.zeros(3), axis=np.array([0.0, 0.0, 1.0]), ref=0.0, armature=0.0, damping=0.0, stiffness=0.0, springref=0.0)
    body = dict(name="b", parent=-1, pos=np.array([0.2, -0.1, 1.0]), quat=np.array([1.0, 0, 0, 0]), joints=[free], mass=1.3, ipos=np.zeros(3), inertia=np.diag(inertia),
                sites=[dict(name="imu", pos=RS, quat=QS)])
    return dict(gravity=tuple(gravity), timestep=0.002, bodies=[body])


def _state():
    quat = R.unit([0.3, -0.6, 0.5, 0.55])
    q = np.r_[[0.3, -0.2, 1.1], quat]
    w_body, v0 = np.array([2.0, -3.0, 1.5]), np.array([1.0, 0.5, -2.0])
    return q, np.r_[v0, w_body], R.qmat(quat), w_body, v0


def _row(out, name):
    a, d = out["adr"][name]
    return out["data"][a:a + d]


def _err_ok(out):
    assert (out["err"] <= 1e-8 * np.maximum(1.0, np.abs(out["data"]))).all(), (out["err"] / np.maximum(1.0, np.abs(out["data"]))).max()


def test_mat2quat_inverts_qmat():
    rng = np.random.default_rng(5)
    for _ in range(50):
        q = R.unit(rng.standard_normal(4))
        got = SR.mat2quat(R.qmat(q))
        assert np.abs(R.sign_like(got, q) - q).max() < 1e-14
    for q in ([0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0]):      # half turns: the trace is -1
        assert np.abs(R.sign_like(SR.mat2quat(R.qmat(np.array(q, dtype=float))), q) - q).max() < 1e-14


def test_free_body_with_given_acceleration():
    tree = _free_body(G)
    q, v, Rb, w_body, v0 = _state()
    qacc = np.array([0.8, -1.1, 2.3, 4.0, -2.5, 3.1])      # the origin's acceleration in the world, the angular acceleration in the body frame
    out = SR.evaluate(tree, q, v, SENSORS, qacc=qacc)
    Rw = Rb @ R.qmat(QS)
    w, r, alpha = Rb @ w_body, Rb @ RS, Rb @ qacc[3:]
    lin = qacc[:3] + np.cross(alpha, r) + np.cross(w, np.cross(w, r)) - G
    assert np.abs(_row(out, "gyro") - R.qmat(QS).T @ w_body).max() < 1e-13
    assert np.abs(_row(out, "velocimeter") - Rw.T @ (v0 + np.cross(w, r))).max() < 1e-13
    assert np.abs(_row(out, "framelinacc") - lin).max() < 1e-8
    assert np.abs(_row(out, "accelerometer") - Rw.T @ lin).max() < 1e-8
    assert np.abs(_row(out, "frameangacc") - alpha).max() < 1e-8
    assert np.abs(_row(out, "framepos") - (q[:3] + r)).max() < 1e-14
    assert np.abs(R.sign_like(_row(out, "framequat"), R.qmul(q[3:], QS)) - R.unit(R.qmul(q[3:], QS))).max() < 1e-14
    _err_ok(out)


def test_free_fall_reads_the_rotation_terms_only():
    """gravity alone, the centre of mass at the body's origin, a sphere's inertia (no torque-free precession): the origin falls with g and the accelerometer is left with the
    centripetal term"""
    tree = _free_body(G, inertia=(0.01, 0.01, 0.01))
    q, v, Rb, w_body, v0 = _state()
    out = SR.evaluate(tree, q, v, SENSORS)
    assert np.abs(out["qacc"] - np.r_[G, 0, 0, 0]).max() < 1e-9
    Rw, w, r = Rb @ R.qmat(QS), Rb @ w_body, Rb @ RS
    assert np.abs(_row(out, "accelerometer") - Rw.T @ np.cross(w, np.cross(w, r))).max() < 1e-8
    assert np.abs(_row(out, "frameangacc")).max() < 1e-8
    assert np.linalg.norm(_row(out, "accelerometer")) > 0.5      # the term is there: |omega|^2 |r_perp|
    _err_ok(out)


def test_turntable_reads_the_centripetal_acceleration():
    hinge = dict(type="hinge", name="spin", pos=np.zeros(3), axis=np.array([0.0, 0.0, 1.0]), ref=0.0, armature=0.0, damping=0.0, stiffness=0.0, springref=0.0)
    body = dict(name="table", parent=-1, pos=np.array([0.0, 0.0, 0.5]), quat=np.array([1.0, 0, 0, 0]), joints=[hinge], mass=2.0, ipos=np.zeros(3), inertia=np.diag([0.02, 0.02, 0.03]),
                sites=[dict(name="imu", pos=np.array([0.25, 0.0, 0.04]), quat=np.array([1.0, 0, 0, 0]))])
    tree = dict(gravity=(0.0, 0.0, -9.81), timestep=0.002, bodies=[body])
    rate, angle = 3.0, 0.7
    out = SR.evaluate(tree, np.array([angle]), np.array([rate]), SENSORS)
    assert abs(out["qacc"][0]) < 1e-12      # no torque about the axis: the rate is constant
    assert np.abs(_row(out, "accelerometer") - np.array([-rate ** 2 * 0.25, 0.0, 9.81])).max() < 1e-8      # towards the axis in the site's own frame, and +g along z
    assert np.abs(_row(out, "gyro") - np.array([0.0, 0.0, rate])).max() < 1e-14
    assert np.abs(_row(out, "velocimeter") - np.array([0.0, rate * 0.25, 0.0])).max() < 1e-14
    _err_ok(out)
