"""tests/dyn_refs.py against itself and against closed forms, before anything is compared with it: its geometric Jacobians are the derivatives of its own kinematics, the mass
matrix and bias of a planar double pendulum and the gyroscopic torque of a free body are the textbook expressions, the kinetic energy v' M v / 2 is the sum of the bodies'
energies taken from finite differences of their poses, and its own error estimate is at most 1e-8 max(1, |value|) on every world of every case of tests/dyn_tree_cases.py."""
import numpy as np
import pytest

import dyn_refs as R
import dyn_tree_cases as T


def _vee(W):
    return 0.5 * np.array([W[2, 1] - W[1, 2], W[0, 2] - W[2, 0], W[1, 0] - W[0, 1]])


def _pose_rates(tree, q, v, h=1e-4):
    """per body the velocity of the centre of mass and the angular velocity along integrate_pos(q, v, t), by central differences of the poses alone (fourth order), and the
    same for the sites"""
    def poses(t):
        k = R.kinematics(tree, R.integrate_pos(tree, q, v, t))
        return k["xipos"], k["xmat"], k["site_xpos"], k["site_xmat"]

    def rate(f):      # f(t) -> array; five-point stencil
        return (8.0 * (f(h) - f(-h)) - (f(2 * h) - f(-2 * h))) / (12.0 * h)

    lin, slin = rate(lambda t: poses(t)[0]), rate(lambda t: poses(t)[2])
    R0, S0 = poses(0.0)[1], poses(0.0)[3]
    ang = np.array([_vee(W @ R0[b].T) for b, W in enumerate(rate(lambda t: poses(t)[1]))])
    sang = np.array([_vee(W @ S0[s].T) for s, W in enumerate(rate(lambda t: poses(t)[3]))]).reshape(-1, 3)
    return lin, ang, slin, sang


@pytest.mark.parametrize("name", T.NAMES)
def test_jacobians_are_the_derivatives_of_the_kinematics(name):
    """column d of a Jacobian is the velocity of the point (the angular velocity of the frame) when dof d alone moves at unit speed -- the free joint's angular dofs turn the
    body about its OWN axes, which integrate_pos does by multiplying on the right"""
    case = T.CASES[name]
    tree, st = case.tree, case.states(3)
    nv = R.layout(tree)[2]
    for i in (0, 2):
        q = st["qpos"][i]
        e = R.evaluate(tree, q, st["qvel"][i], levels=1)
        worst = 0.0
        for d in range(nv):
            lin, ang, slin, sang = _pose_rates(tree, q, np.eye(nv)[d])
            worst = max(worst, np.abs(lin - e["com_jacp"][:, :, d]).max(), np.abs(ang - e["com_jacr"][:, :, d]).max(), np.abs(slin - e["site_jacp"][:, :, d]).max(),
                        np.abs(sang - e["site_jacr"][:, :, d]).max())
        print(name, "world", i, "Jacobian vs finite differences", worst)
        assert worst < 1e-9, (name, i, worst)


@pytest.mark.parametrize("name", T.NAMES)
def test_kinetic_energy_is_the_sum_over_the_bodies(name):
    case = T.CASES[name]
    tree, st = case.tree, case.states(3)
    q, v = st["qpos"][2], st["qvel"][2]
    e = R.evaluate(tree, q, v, levels=1)
    lin, ang, _, _ = _pose_rates(tree, q, v)
    m = np.array([b["mass"] for b in tree["bodies"]])
    arm = np.concatenate([[j["armature"]] * (6 if j["type"] == "free" else 1) for b in tree["bodies"] for j in b["joints"]])
    bodies = 0.5 * float((m * (lin ** 2).sum(axis=1)).sum() + np.einsum("bk,bkl,bl->", ang, e["Iw"], ang)) + 0.5 * float((arm * v ** 2).sum())
    whole = 0.5 * float(v @ e["M"] @ v)
    print(name, "energy", whole, bodies)
    assert abs(whole - bodies) < 1e-8 * max(1.0, whole)


def _pendulum(m1, m2, l1, l2, g):
    """two point masses on massless rods in the x-z plane, hinges about +y, gravity along -z; at q = 0 both rods point along +x"""
    point = lambda name, parent, x, m, l: dict(name=name, parent=parent, pos=[x, 0.0, 0.0], quat=[1.0, 0, 0, 0], mass=m, ipos=[l, 0.0, 0.0], inertia=np.zeros((3, 3)), sites=[],
                                               joints=[dict(type="hinge", name="j" + name, pos=[0.0, 0, 0], axis=[0.0, 1.0, 0.0], ref=0.0, armature=0.0, damping=0.0, stiffness=0.0, springref=0.0)])
    return dict(gravity=(0.0, 0.0, -g), timestep=0.002, bodies=[point("a", -1, 0.0, m1, l1), point("b", 0, l1, m2, l2)])


@pytest.mark.parametrize("q,v", [((0.3, -0.7), (1.1, -2.3)), ((-1.2, 2.1), (-3.0, 0.4)), ((0.0, 0.0), (0.0, 0.0)), ((2.5, 0.9), (4.0, 5.0))])
def test_planar_double_pendulum(q, v):
    """the textbook double pendulum.  A turn by t about +y takes +x to (cos t, 0, -sin t): z1 = -l1 sin t1, z2 = z1 - l2 sin(t1 + t2)"""
    m1, m2, l1, l2, g = 0.7, 0.4, 0.35, 0.25, 9.81
    e = R.evaluate(_pendulum(m1, m2, l1, l2, g), np.array(q), np.array(v))
    c2, s2 = np.cos(q[1]), np.sin(q[1])
    M = np.array([[(m1 + m2) * l1 ** 2 + m2 * l2 ** 2 + 2 * m2 * l1 * l2 * c2, m2 * l2 ** 2 + m2 * l1 * l2 * c2], [m2 * l2 ** 2 + m2 * l1 * l2 * c2, m2 * l2 ** 2]])
    cor = np.array([-m2 * l1 * l2 * s2 * (2 * v[0] * v[1] + v[1] ** 2), m2 * l1 * l2 * s2 * v[0] ** 2])
    grav = np.array([-(m1 + m2) * g * l1 * np.cos(q[0]) - m2 * g * l2 * np.cos(q[0] + q[1]), -m2 * g * l2 * np.cos(q[0] + q[1])])      # dV/dq
    assert np.abs(e["M"] - M).max() < 1e-14
    assert np.abs(e["qfrc_bias"] - (cor + grav)).max() < 1e-9, (e["qfrc_bias"], cor + grav)
    assert np.abs(e["qacc_smooth"] - np.linalg.solve(M, -(cor + grav))).max() < 1e-8


def test_pendulum_ref_shifts_the_angle():
    """a hinge with ref = r at qpos = r + t stands where the same hinge with ref = 0 stands at qpos = t"""
    a, b = _pendulum(0.7, 0.4, 0.35, 0.25, 9.81), _pendulum(0.7, 0.4, 0.35, 0.25, 9.81)
    b["bodies"][0]["joints"][0]["ref"], b["bodies"][1]["joints"][0]["ref"] = 0.4, -1.1
    ea, eb = R.evaluate(a, np.array([0.3, -0.7]), np.array([1.0, 2.0])), R.evaluate(b, np.array([0.7, -1.8]), np.array([1.0, 2.0]))
    for k in ("xpos", "xmat", "M", "qfrc_bias"):
        assert np.abs(ea[k] - eb[k]).max() < 1e-12, k
    assert np.allclose(R.qpos0(b), [0.4, -1.1])


def test_free_body_gyroscopic_torque_and_euler_equations():
    """a free body whose frame sits at its centre of mass: the bias on the angular dofs is omega x I omega in the body's own frame and -m g on the linear ones; without
    gravity the acceleration is Euler's I domega = -(omega x I omega) -- with an inertia that is not diagonal and an attitude far from the identity"""
    rng = np.random.default_rng(5)
    Rm = R.qmat(R.unit(rng.standard_normal(4)))
    I = Rm @ np.diag([0.004, 0.011, 0.013]) @ Rm.T
    g = np.array([1.5, -2.0, -9.0])
    free = dict(type="free", name="root", pos=[0.0, 0, 0], axis=[0.0, 0, 1], ref=0.0, armature=0.0, damping=0.0, stiffness=0.0, springref=0.0)
    tree = dict(gravity=g, timestep=0.002, bodies=[dict(name="a", parent=-1, pos=[0.0, 0, 1], quat=[1.0, 0, 0, 0], joints=[free], mass=1.3, ipos=[0.0, 0, 0], inertia=I, sites=[])])
    q = np.r_[0.2, -0.1, 1.2, R.unit([0.3, -0.6, 0.5, 0.55])]
    w = 10.0 * R.unit(rng.standard_normal(3))
    v = np.r_[0.5, -1.0, 2.0, w]
    e = R.evaluate(tree, q, v)
    assert np.abs(e["qfrc_bias"][3:] - np.cross(w, I @ w)).max() < 1e-9
    assert np.abs(e["qfrc_bias"][:3] + 1.3 * g).max() < 1e-9
    assert np.abs(e["qacc_smooth"][3:] - np.linalg.solve(I, -np.cross(w, I @ w))).max() < 1e-7 and np.abs(e["qacc_smooth"][:3] - g).max() < 1e-9
    # the world-frame reading of the same velocity is a different motion: the attitude is far from the identity
    world = R.unit(R.qmul(R.qexp(1e-3 * w), q[3:]))
    assert np.abs(R.sign_like(R.integrate_pos(tree, q, v, 1e-3)[3:], world) - world).max() > 1e-3


def test_joints_of_one_body_apply_in_order():
    """slide along x, then a hinge about z through the origin of the moved frame: the body's origin is at (d, 0, 0) whatever the angle.  The other order swings the slide
    direction round with the hinge."""
    j = lambda t, ax: dict(type=t, name=t, pos=[0.0, 0, 0], axis=ax, ref=0.0, armature=0.0, damping=0.0, stiffness=0.0, springref=0.0)
    body = lambda joints: dict(gravity=(0, 0, -9.81), timestep=0.002, bodies=[dict(name="a", parent=-1, pos=[0.0, 0, 0], quat=[1.0, 0, 0, 0], joints=joints, mass=1.0, ipos=[0.0, 0, 0],
                                                                                    inertia=np.eye(3), sites=[])])
    a = R.kinematics(body([j("slide", [1.0, 0, 0]), j("hinge", [0.0, 0, 1])]), np.array([0.5, np.pi / 2]))
    b = R.kinematics(body([j("hinge", [0.0, 0, 1]), j("slide", [1.0, 0, 0])]), np.array([np.pi / 2, 0.5]))
    assert np.abs(a["xpos"][0] - [0.5, 0, 0]).max() < 1e-15 and np.abs(b["xpos"][0] - [0, 0.5, 0]).max() < 1e-15
    assert np.abs(a["xmat"][0] - b["xmat"][0]).max() < 1e-15


@pytest.mark.parametrize("name,n", T.RUNS)
def test_the_references_own_error_is_small(name, n):
    """a condition on the reference alone: every estimate of every field of every world is at most 1e-8 max(1, |value|), a hundredth of the ceiling the oracle is held to"""
    ref = T.reference(name, n)
    worst = {}
    for k, err in ref["err"].items():
        ratio = err / (1e-8 * np.maximum(1.0, np.abs(ref[k])))
        worst[k] = float(ratio.max()) if ratio.size else 0.0
    print(name, n, "estimate / (1e-8 max(1, |value|)):", " ".join(f"{k} {v:.1e}" for k, v in worst.items()), "| Richardson on accelerations",
          max(r["acc"] for r in ref["richardson"]))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_solids_and_spellings_closed_forms():
    """the generator's own conversions: a capsule of zero length is a sphere, of zero radius... a thin rod; a box built from eight boxes; euler zyx by hand"""
    vs, Is = T.solid("sphere", (0.05,))
    vc, Ic = T.solid("capsule", (0.05, 0.0))
    assert abs(vs - vc) < 1e-18 and np.abs(Is - Ic).max() < 1e-18
    vb, Ib = T.solid("box", (0.06, 0.04, 0.02))
    parts = [(vb / 8, np.array([sx * 0.03, sy * 0.02, sz * 0.01]), T.solid("box", (0.03, 0.02, 0.01))[1]) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    m, c, I = T.combine(parts)
    assert abs(m - vb) < 1e-18 and np.abs(c).max() < 1e-18 and np.abs(I - Ib).max() < 1e-18
    # a capsule against a numerical integral of its solid of revolution: I_zz = pi/2 int r(z)^4 dz, I_xx = int (pi r^4 / 4 + pi r^2 z^2) dz
    r, h = 0.03, 0.07
    z = np.linspace(-(h + r), h + r, 400001)
    rad = np.where(np.abs(z) <= h, r, np.sqrt(np.maximum(0.0, r * r - (np.abs(z) - h) ** 2)))
    vol, I = T.solid("capsule", (r, h))
    trapz = lambda y: float(((y[1:] + y[:-1]) * np.diff(z)).sum() / 2.0)
    assert abs(trapz(np.pi * rad ** 2) - vol) < 1e-9 * vol
    assert abs(trapz(np.pi / 2 * rad ** 4) - I[2, 2]) < 1e-8 * I[2, 2] and abs(trapz(np.pi / 4 * rad ** 4 + np.pi * rad ** 2 * z ** 2) - I[0, 0]) < 1e-8 * I[0, 0]
    # eulerseq "zyx", intrinsic: about z, then about the new y, then about the newest x
    a, b, c = np.radians([35.0, -50.0, 20.0])
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    assert np.abs(R.qmat(T.ori_quat(("euler", (35.0, -50.0, 20.0)), np.pi / 180, "zyx")) - Rz @ Ry @ Rx).max() < 1e-15
    assert np.abs(R.qmat(T.ori_quat(("euler", (35.0, -50.0, 20.0)), np.pi / 180, "xyz")) - Rz @ Ry @ Rx).max() > 0.1
    zq = R.qmat(T.ori_quat(("zaxis", (0.5, 0.3, -0.7)), 1.0, "xyz"))
    assert np.abs(zq[:, 2] - R.unit([0.5, 0.3, -0.7])).max() < 1e-15
    xy = R.qmat(T.ori_quat(("xyaxes", (1.0, 0.4, -0.3, 0.2, 1.0, 0.5)), 1.0, "xyz"))
    assert np.abs(xy[:, 0] - R.unit([1.0, 0.4, -0.3])).max() < 1e-15 and abs(xy[:, 1] @ xy[:, 0]) < 1e-15 and xy[:, 1] @ [0.2, 1.0, 0.5] > 0 and np.abs(xy @ xy.T - np.eye(3)).max() < 1e-15
