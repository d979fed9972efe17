"""tests/constraint_refs.py held to closed forms: the scalar minimiser of one limit row, the sticking and slipping regimes of one friction-loss row, a stiff joint equality
against direct elimination, a position actuator against the passive spring of dyn_refs, RK4 of a frictionless pendulum against a fine-step integration with the observed
fourth order, and the KKT certificate of every generated world the other files use."""
import numpy as np
import pytest

import constraint_cases as CC
import constraint_refs as K
import dyn_refs as R


def _link(name, parent, jtype, axis, mass=0.7, inertia=(0.02, 0.03, 0.04), ipos=(0.0, 0.0, 0.0), **joint):
    j = dict(type=jtype, name="j_" + name, pos=np.zeros(3), axis=np.asarray(axis, dtype=np.float64), ref=0.0, armature=0.0, damping=0.0, stiffness=0.0, springref=0.0, **joint)
    return dict(name=name, parent=parent, pos=np.zeros(3), quat=np.array([1.0, 0, 0, 0]), joints=[j], mass=mass, ipos=np.asarray(ipos, dtype=np.float64), inertia=np.diag(inertia), sites=[])


def _tree(bodies, gravity=(0.0, 0.0, 0.0), h=0.002, **kw):
    return dict(gravity=gravity, timestep=h, bodies=bodies, **kw)


@pytest.mark.parametrize("solref,solimp,margin", [((0.02, 1.0), K.SOLIMP, 0.0), ((0.001, 1.0), (0.85, 0.97, 0.002, 0.4, 3.0), 0.01), ((-1500.0, -50.0), K.SOLIMP, 0.0)])
@pytest.mark.parametrize("side", [0, 1])
def test_one_hinge_inside_its_limit(solref, solimp, margin, side):
    """gravity off, a hinge beyond its limit by p with velocity v and a spring pulling it on: qacc = (m a_s + D aref) / (m + D) when the row pushes, a_s when it does not"""
    I, p, h = 0.04, 2e-3, 0.002
    for v in (-0.5, 0.3, 40.0):
        tree = _tree([_link("a", -1, "hinge", (0, 0, 1), range=(-0.3, 0.4), margin=margin, solreflimit=solref, solimplimit=solimp)], h=h)
        tree["bodies"][0]["joints"][0].update(stiffness=3.0, springref=0.1)
        q = -0.3 - p if side == 0 else 0.4 + p
        f = K.forward(tree, [q], [v])
        sign, dist = (1.0, q + 0.3) if side == 0 else (-1.0, 0.4 - q)
        a_s = -3.0 * (q - 0.1) / I
        d = K.impedance(solimp, dist - margin)
        dmax = solimp[1]
        k, b = (1.0 / (dmax ** 2 * max(solref[0], 2 * h) ** 2 * solref[1] ** 2), 2.0 / (dmax * max(solref[0], 2 * h))) if solref[0] > 0 else (-solref[0] / dmax ** 2, -solref[1] / dmax)
        aref = -b * sign * v - k * d * (dist - margin)
        D = d / ((1.0 - d) * (1.0 / I))
        want = sign * (I * sign * a_s + D * aref) / (I + D) if sign * a_s - aref < 0 else a_s
        assert f["nefc"] == 1 and abs(f["efc_aref"][0] - aref) <= 1e-12 * abs(aref) and abs(f["efc_D"][0] - D) <= 1e-12 * D
        assert abs(f["qacc"][0] - want) <= 1e-12 * max(1.0, abs(want)), (v, f["qacc"], want)
    assert K.forward(tree, [0.0], [1.0])["nefc"] == 0


def test_impedance_curve():
    s = (0.85, 0.97, 0.002, 0.4, 3.0)
    assert K.impedance(s, 0.0) == 0.85 and K.impedance(s, 0.002) == 0.97 and K.impedance(s, -1.0) == 0.97
    x = 0.3      # below the midpoint: y = x^p / mid^(p - 1); above: 1 - (1 - x)^p / (1 - mid)^(p - 1)
    assert abs(K.impedance(s, x * 0.002) - (0.85 + 0.12 * x ** 3 / 0.4 ** 2)) < 1e-15
    assert abs(K.impedance(s, -0.7 * 0.002) - (0.85 + 0.12 * (1 - 0.3 ** 3 / 0.6 ** 2))) < 1e-15
    assert abs(K.impedance(s, 0.4 * 0.002) - (0.85 + 0.12 * 0.4)) < 1e-15      # the curve passes through (mid, mid)
    assert K.impedance((2.0, -1.0, 0.001, 0.5, 2.0), 0.0005) == K.impedance((K.MAXIMP, K.MINIMP, 0.001, 0.5, 2.0), 0.0005)      # the clamps
    assert K.impedance((0.9, 0.9, 0.001, 0.5, 2.0), 0.3) == 0.9 and K.impedance((0.8, 0.9, 0.0, 0.5, 2.0), 0.3) == pytest.approx(0.85)


def test_one_slide_with_friction_loss():
    """a slide of mass m pushed by a spring force F: it sticks (the row holds a = aref exactly up to its softness) while |m (a_s - aref)| is small, and beyond the Huber zone
    the force is exactly -+f"""
    m, fl, h = 0.7, 0.4, 0.002
    tree = _tree([_link("s", -1, "slide", (1, 0, 0), mass=m, frictionloss=fl)], h=h)
    j = tree["bodies"][0]["joints"][0]
    d = 0.9      # the impedance at pos = 0: dmin
    Rr = (1 - d) / d * (1.0 / m)
    b = 2.0 / (0.95 * 0.02)
    for F, v in ((0.1, 0.0), (-0.2, 1e-4), (3.0, 0.0), (-3.0, 0.0), (0.1, 2.0), (0.1, -2.0)):
        j.update(stiffness=1.0, springref=F)      # at q = 0 the spring pushes with F
        f = K.forward(tree, [0.0], [v])
        a_s, aref = F / m, -b * v
        quad = (m * a_s + aref / Rr) / (m + 1.0 / Rr)
        if abs(quad - aref) <= Rr * fl:
            assert f["efc_piece"][0] == 0 and abs(f["qacc"][0] - quad) < 1e-12 * max(1.0, abs(quad))
            assert abs(f["efc_force"][0]) < fl
        else:
            s = np.sign(quad - aref)
            assert f["efc_piece"][0] == s and f["efc_force"][0] == -s * fl and abs(f["qacc"][0] - (a_s - s * fl / m)) < 1e-12 * max(1.0, abs(a_s))
        assert f["efc_aref"][0] == pytest.approx(aref) and f["efc_R"][0] == pytest.approx(Rr)
    assert {-1, 0, 1} == {int(K.forward(tree, [0.0], [v])["efc_piece"][0]) for v in (0.0, 2.0, -2.0)}


def test_two_hinges_tied_by_a_linear_equality():
    """q1 = c q2 exactly enforced gives a = (x'M x)^-1 x' tau x with x = (c, 1); the soft row's answer differs by its documented softness: the row's residual
    acceleration J a - aref = -R f, so the violation is bounded by R |f| = (1 - d) / d diagApprox |f|"""
    c = -1.2
    bodies = [_link("a", -1, "hinge", (0, 0, 1), ipos=(0.1, 0, 0)), _link("b", -1, "hinge", (0, 1, 0), mass=0.4, ipos=(0.05, 0, 0.02))]
    bodies[0]["joints"][0].update(stiffness=2.0, springref=0.5)
    tree = _tree(bodies, gravity=(0.0, 0.0, -9.81), equalities=[dict(joint1="j_a", joint2="j_b", polycoef=(0.0, c, 0.0, 0.0, 0.0), solimp=(0.9999, 0.9999, 0.001, 0.5, 2.0))])
    q = np.array([c * 0.2, 0.2])
    f = K.forward(tree, q, np.zeros(2))      # on the curve and at rest: aref = 0, the constraint asks for J a = 0
    x = np.array([c, 1.0])
    hard = x * (x @ f["qfrc_smooth"]) / (x @ f["M"] @ x)
    soft = f["efc_R"][0] * abs(f["efc_force"][0])
    assert f["nefc"] == 1 and abs(f["efc_pos"][0]) < 1e-15 and np.allclose(f["efc_J"][0], [1.0, -c])
    assert abs(f["efc_J"][0] @ f["qacc"] + f["efc_R"][0] * f["efc_force"][0] - f["efc_aref"][0]) < 1e-9
    assert soft < 1e-2 and np.abs(f["qacc"] - hard).max() <= 2.0 * soft * np.abs(x).max(), (f["qacc"], hard, soft)
    assert np.abs(f["qacc"] - hard).max() > 0      # and it IS soft
    quart = dict(joint1="j_a", joint2="j_b", polycoef=(0.01, 0.8, -0.3, 0.2, -0.1))
    g = K.forward(_tree(bodies, equalities=[quart]), [0.3, 0.4], np.zeros(2))
    assert g["efc_pos"][0] == pytest.approx(0.3 - (0.01 + 0.8 * 0.4 - 0.3 * 0.16 + 0.2 * 0.064 - 0.1 * 0.0256))
    assert g["efc_J"][0][1] == pytest.approx(-(0.8 - 2 * 0.3 * 0.4 + 3 * 0.2 * 0.16 - 4 * 0.1 * 0.064))
    assert K.forward(_tree(bodies, equalities=[dict(quart, active=False)]), [0.3, 0.4], np.zeros(2))["nefc"] == 0


def test_position_actuator_is_a_spring():
    kp, target = 25.0, 0.3
    mk = lambda **kw: _link("a", -1, "hinge", (0.2, 0.3, 1.0) / np.linalg.norm((0.2, 0.3, 1.0)), ipos=(0.1, 0.02, 0), **kw)
    spring = _tree([mk()], gravity=(1.5, -2.0, -9.0))
    spring["bodies"][0]["joints"][0].update(stiffness=kp, springref=target)
    act = _tree([mk()], gravity=(1.5, -2.0, -9.0), actuators=[dict(joint="j_a", gear=1.0, gain=kp, bias=(0.0, -kp, 0.0), ctrlrange=None, forcerange=None)])
    for q, v in ((0.7, 2.0), (-0.4, -1.0)):
        a, b = K.forward(act, [q], [v], [target]), R.evaluate(spring, [q], [v])
        assert a["qfrc_actuator"][0] == pytest.approx(-kp * (q - target)) and abs(a["qacc"][0] - b["qacc"][0]) <= 1e-12 * abs(b["qacc"][0])
    geared = _tree([mk()], actuators=[dict(joint="j_a", gear=2.0, gain=8.0, bias=(0.4, -6.0, -0.8), ctrlrange=(-0.6, 0.8), forcerange=(-3.0, 2.5))] * 2)
    f = K.actuation(geared, [0.1], [0.5], [5.0, 0.2])
    one = lambda u: 2.0 * min(2.5, max(-3.0, 8.0 * min(0.8, max(-0.6, u)) + 0.4 - 6.0 * 0.2 - 0.8 * 1.0))
    assert f["qfrc_actuator"][0] == pytest.approx(one(5.0) + one(0.2)) and one(5.0) == 5.0      # two on one joint add; the first one is force-clamped BEFORE the gear


def test_rk4_of_a_frictionless_pendulum_has_fourth_order():
    tree = _tree([_link("p", -1, "hinge", (0, 1, 0), ipos=(0.0, 0.0, -0.3))], gravity=(0.0, 0.0, -9.81), h=0.02, integrator="RK4")
    T_end = 0.32

    def run(h):
        t = dict(tree, timestep=h)
        q, v, _ = K.step(t, [1.0], [0.5], nstep=int(round(T_end / h)), levels=4)
        return np.r_[q, v]

    fine = run(0.02 / 16)
    e1, e2 = np.abs(run(0.02) - fine).max(), np.abs(run(0.01) - fine).max()
    order = np.log2(e1 / e2)
    print("rk4 errors", e1, e2, "order", order)
    assert 3.6 < order < 4.6 and e1 < 1e-6
    euler = dict(tree, integrator="Euler", timestep=0.01)
    qe, ve, _ = K.step(euler, [1.0], [0.5], nstep=32)
    assert np.abs(np.r_[qe, ve] - fine).max() > 100 * e2      # and Euler is not


def test_rk4_has_no_implicit_damping_and_euler_has():
    bodies = [_link("p", -1, "hinge", (0, 1, 0), ipos=(0.0, 0.0, -0.3))]
    bodies[0]["joints"][0].update(damping=5.0)
    h, I = 0.01, 0.03 + 0.7 * 0.09      # about the y axis, through the joint
    _, ve, _ = K.step(_tree(bodies, h=h), [0.0], [1.0])
    assert ve[0] == pytest.approx(1.0 + h * (-5.0) / (I + h * 5.0))
    _, vr, _ = K.step(_tree(bodies, h=h, integrator="RK4"), [0.0], [1.0])
    lam = -5.0 / I * h
    assert vr[0] == pytest.approx(1.0 + lam + lam ** 2 / 2 + lam ** 3 / 6 + lam ** 4 / 24)


def test_invweights_of_a_free_body_are_the_means():
    m, I = 1.3, np.diag([0.004, 0.011, 0.013])
    free = dict(type="free", name="root", pos=np.zeros(3), axis=np.array([0.0, 0, 1]), ref=0.0, armature=0.0, damping=0.0, stiffness=0.0, springref=0.0)
    body = dict(name="f", parent=-1, pos=np.array([0.1, 0.2, 1.0]), quat=R.unit([0.3, -0.6, 0.5, 0.55]), joints=[free], mass=m, ipos=np.zeros(3), inertia=I, sites=[])
    w = K.constants(_tree([body]))["dof_invweight0"]
    assert np.allclose(w[:3], 1.0 / m) and np.allclose(w[3:], np.mean(1.0 / np.diag(I)))


@pytest.mark.parametrize("name,n", CC.RUNS)
def test_every_generated_world_has_its_certificate(name, n):
    worst = 0.0
    for r in CC.reference(name, n):
        worst = max(worst, r["kkt"] / r["kkt_scale"])
        f, piece = K.row_forces(dict(kind=r["efc_kind"], J=r["efc_J"], aref=r["efc_aref"], D=r["efc_D"], R=r["efc_R"], floss=r["efc_floss"]), r["qacc"])
        assert np.array_equal(piece, r["efc_piece"]) and np.array_equal(f, r["efc_force"])
        assert np.abs(r["M"] @ (r["qacc"] - r["qacc_smooth"]) - r["efc_J"].T @ f).max(initial=0.0) <= K.CERT * r["kkt_scale"]
    print(name, n, "KKT residual / scale", worst)
    assert worst <= K.CERT
