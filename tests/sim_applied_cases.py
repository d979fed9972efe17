"""Applied forces of grx.BatchedSim (tests/test_cpu_sim_applied.py, tests/test_gpu_sim_applied.py): the scene, the applied rows and the references.  Plain Python and numpy.

The fp64 oracle has no qfrc_applied / xfrc_applied.  Three exact equivalences make it the reference all the same:

a. motor twin ..... a gear-g <motor> without ctrlrange on dof d: qfrc_applied[d] = u is the same model as u / g added to that motor's ctrl.
b. gravity twin ... xfrc_applied[b] = (m_b a, 0) on every body b is the same model as gravity g + a (m_b: the COMPILED body_mass, merged static children included).
                    The twins are the same MODEL, not the same bookkeeping: the twin books u under qfrc_actuator and the a-term under qfrc_bias, MjData books both under
                    neither (qfrc_bias, qfrc_passive and qfrc_actuator do not contain the applied terms).  twin_world moves the two exactly known terms back before a comparison.
c. closed form .... with a site on every movable body's centre of mass, Q = qfrc_applied + sum_b jacp_b' f_b + jacr_b' t_b from OracleSim.jac_site of those sites, and one pass
                    gives qfrc_smooth = oracle.qfrc_smooth + Q, qacc_smooth = oracle.qacc_smooth + M^-1 Q and, without constraint rows, qacc = that qacc_smooth.  For forces
                    on bodies whose dofs all carry gear-1 motors, step(1) of an Euler model equals the oracle's step(1) with ctrl += Q taken from forward() at the same state.

Scene push: a 3-joint chain (two hinges and a slide, geoms off the body frames so that body_ipos != 0, a jointless massive child `lump` that the compiler merges into link l2,
a gear-1 <motor> without ctrlrange on every joint) and a free box on a plane with its geom off the body frame, pressed in 0.3 .. 3 mm or held above the plane (worlds with
i mod 5 in UP: no constraint rows at all).  One site sits on every movable body's centre of mass: the MJCF is compiled once without them to read body_ipos.
rk4 and pile are the scenes of tests/sim_cases.py.

Applied values per world from a seeded generator, rounded to fp32: the twin acceleration a has a lateral part of LATERAL[i mod 5] times g (the push on the box is that many
times its weight: it sticks for 0.3 and 0.8 and slides for 2.5, friction 1) in a random direction and |a_z| <= 3 m/s^2; qfrc_applied within +-1; the closed-form rows hold
forces within +-2 N (box: +-0.5 N) and torques within +-0.5 N m."""
import numpy as np

import engine_matrix_cases as C
import sim_cases as S
import sim_dyn_cases as D
import sim_params_cases as P

N = S.N_WORLDS
UP = (0, 3)                                # i mod 5 of the worlds whose box is held above the plane (nefc == 0)
LATERAL = (0.0, 0.3, 0.8, 1.5, 2.5)        # lateral push in units of the weight, by i mod 5
_BOX = 0.05
CHAIN_BODIES = ("l1", "l2", "l3")
MOVABLE = CHAIN_BODIES + ("box",)
COM_SITES = tuple("com_" + b for b in MOVABLE)


def _push_xml(com=None):
    site = lambda b: "" if com is None else f'<site name="com_{b}" pos="{com[b][0]!r} {com[b][1]!r} {com[b][2]!r}"/>'
    return f"""<mujoco>
  <compiler angle="radian"/>
  <option timestep="0.002"/>
  <worldbody>
    <geom name="floor" type="plane" size="2 2 0.1" condim="3"/>
    <body name="l1" pos="0 0 0.6">
      <joint name="h1" type="hinge" axis="0 1 0" damping="0.2" armature="0.01"/>
      <geom type="capsule" fromto="0 0.01 0 0.2 0.01 0.05" size="0.02" mass="0.5" contype="0" conaffinity="0"/>
      {site("l1")}
      <body name="l2" pos="0.2 0 0.05">
        <joint name="h2" type="hinge" axis="0 0 1" damping="0.1" armature="0.01"/>
        <geom type="box" size="0.08 0.02 0.02" pos="0.08 0.03 0" mass="0.3" contype="0" conaffinity="0"/>
        {site("l2")}
        <body name="lump" pos="0.05 -0.04 0.02"><geom type="sphere" size="0.03" mass="0.6" contype="0" conaffinity="0"/></body>
        <body name="l3" pos="0.16 0 0">
          <joint name="s3" type="slide" axis="1 0 0" damping="0.5" armature="0.01"/>
          <geom type="capsule" fromto="0 0.01 0 0.1 0.01 0.02" size="0.015" mass="0.2" contype="0" conaffinity="0"/>
          {site("l3")}
        </body>
      </body>
    </body>
    <body name="box" pos="0.6 0.3 {_BOX}">
      <freejoint name="boxj"/>
      <geom name="boxg" type="box" size="{_BOX} {_BOX} {_BOX}" pos="0.01 -0.015 0" mass="0.1" condim="3"/>
      {site("box")}
    </body>
  </worldbody>
  <actuator>
    <motor name="m1" joint="h1" gear="1"/>
    <motor name="m2" joint="h2" gear="1"/>
    <motor name="m3" joint="s3" gear="1"/>
  </actuator>
</mujoco>"""


class _PushScene(S.Scene):
    """the MJCF with the centre-of-mass sites needs body_ipos of the compiled model: it is written on first use"""

    def __init__(self):
        super().__init__("push", None, 21, compile_kwargs=dict(keep_sites=COM_SITES))

    @property
    def xml(self):
        if self._xml is None:
            bare = S.Scene("push_bare", _push_xml(), 21).model
            ipos = np.asarray(bare.tables["body_ipos"], dtype=np.float64).reshape(-1, 3)
            self._xml = _push_xml({b: [float(x) for x in ipos[bare.names["body"][b]]] for b in MOVABLE})
        return self._xml

    @xml.setter
    def xml(self, text):
        self._xml = text


def _push_states(model, n, seed):
    nq, nv, nu, nm = S._dims(model)
    q, v, u = np.zeros((n, nq)), np.zeros((n, nv)), np.zeros((n, nu))
    for i in range(n):
        r = S._world_rng(seed, i)
        q[i, :3] = r.uniform([-1.0, -1.2, -0.03], [1.0, 1.2, 0.05])
        v[i, :3] = [0.5, 0.5, 0.1] * r.standard_normal(3)
        yaw = r.uniform(-np.pi, np.pi)
        z = _BOX + 0.02 + 0.01 * r.uniform() if i % 5 in UP else _BOX - r.uniform(3e-4, 3e-3)
        q[i, 3:6] = [0.6 + 0.05 * r.standard_normal(), 0.3 + 0.05 * r.standard_normal(), z]
        q[i, 6:10] = C.axis_angle([0, 0, 1], yaw)
        v[i, 3:9] = np.r_[0.05 * r.standard_normal(2), 0.0, 0.0, 0.0, 0.2 * r.standard_normal()]
        u[i] = 0.5 * r.standard_normal(nu)
    return dict(qpos=q, qvel=v, ctrl=u, mocap_pos=np.zeros((n, nm, 3)), mocap_quat=np.zeros((n, nm, 4)))


S._STATES.setdefault("push", _push_states)
SCENES = dict(push=_PushScene(), rk4=S.SCENES["rk4"], pile=S.SCENES["pile"])
for _k in ("push",):
    D.SCENES.setdefault(_k, SCENES[_k])
D.JAC_SITES.setdefault("push", ("com_l3", "com_box"))
TWIN_CASES = [(s, k, N) for s in ("push", "rk4") for k in (0, 1, 4)] + [("push", 1, 13)]      # item 1 of the GPU file
PILE_CASES = [("pile", 1, N), ("pile", 4, N)]
# (scene, world) -> which redraw of the applied rows: none was needed (every world of every case passes the preconditions of tests/test_cpu_sim_applied.py)
REDRAWN = {}


def _rng(scene, i, what):
    return np.random.default_rng([0xF0C, scene.seed, what, i] + ([REDRAWN[scene.name, i]] if (scene.name, i) in REDRAWN else []))


def body_mass(scene):
    return C.f32(np.asarray(scene.model.tables["body_mass"], dtype=np.float64).reshape(-1))


def gravity(scene):
    return P.nominal(scene, "gravity")


def motors(scene):
    """(dof, gear) of every actuator: all of these scenes' actuators are <motor>s without ctrlrange on a hinge or slide joint"""
    m = scene.model
    tid = np.asarray(m.tables["act_trnid"]).reshape(-1)
    gear = C.f32(np.asarray(m.tables["act_gear"], dtype=np.float64).reshape(-1))
    dofadr = np.asarray(m.tables["jnt_dofadr"]).reshape(-1)
    return [(int(dofadr[tid[a]]), float(gear[a])) for a in range(m.dim("nu"))]


_TWINS = {}


def twin_rows(scene, n=N):
    """the applied rows of twins (a) and (b): dict(accel [n,3], qfrc_applied [n,nv] (motor dofs only), xfrc_applied [n,nbody,6] = (m_b a, 0)) as fp32 values"""
    key = (scene.name, n)
    if key not in _TWINS:
        nv, nb = scene.model.dim("nv"), scene.model.dim("nbody")
        g = np.linalg.norm(gravity(scene))
        acc, qf = np.zeros((n, 3)), np.zeros((n, nv))
        for i in range(n):
            r = _rng(scene, i, 1)
            th = r.uniform(-np.pi, np.pi)
            acc[i] = [LATERAL[i % 5] * g * np.cos(th), LATERAL[i % 5] * g * np.sin(th), r.uniform(-3.0, 3.0)]
            for d, _ in motors(scene):
                qf[i, d] = r.uniform(-1.0, 1.0)
        acc, qf = C.f32(acc), C.f32(qf)
        x = np.zeros((n, nb, 6))
        x[:, :, :3] = body_mass(scene)[None, :, None] * acc[:, None, :]
        x[:, 0] = 0.0
        _TWINS[key] = dict(accel=acc, qfrc_applied=qf, xfrc_applied=C.f32(x))
    return _TWINS[key]


def twin_reference_inputs(scene, rows, st, mass=None, grav=None):
    """what the oracle twin is given: (gravity rows [n,3], ctrl [n,nu]).  The device adds fp32(m_b a) to every body; the twin's gravity is g + a, so the two models differ by
    the rounding of m_b a to fp32, a relative 6e-8 of a force that is itself at most 2.7 times the weight: far below every bound here (and the same for every test).
    mass / grav: per-world tables of the parameter case ([n,nbody], [n,3])"""
    n = len(rows["accel"])
    g = np.broadcast_to(gravity(scene), (n, 3)) if grav is None else np.asarray(grav, dtype=np.float64)
    ctrl = np.array(st["ctrl"], dtype=np.float64, copy=True)
    for a, (d, gear) in enumerate(motors(scene)):
        ctrl[:, a] += rows["qfrc_applied"][:, d] / gear
    return g + rows["accel"], ctrl


def world(scene, orc, st, i, nstep, ids=(), qpos=None):
    """sim_dyn_cases.oracle_world on the oracle `orc`, plus xipos and the centre-of-mass Jacobians' raw material (orc is left at the answer)"""
    with P.standing_in(scene, orc):
        out = D.oracle_world(scene, st, i, nstep, tuple(ids), qpos=qpos)
    out["xipos"] = orc.xipos.reshape(-1, 3).copy()
    return out


def twin_world(scene, orc, st, i, nstep, rows, ids=(), qpos=None):
    """world() on a twin oracle, with the two fields put back where MuJoCo's definition has them.  The twin's qfrc_actuator holds qfrc_applied (gear x (u1 + u2 / gear) on a
    motor without clamps) and its qfrc_bias holds -sum_b jacp_b' m_b a (the gravity term of the bias force): the device's hold neither, as MjData's do not.  Both terms
    are exact, taken from the twin's own last pass: qfrc_actuator -= qfrc_applied, qfrc_bias += Q(xfrc_applied).  Everything else is compared as the twin has it."""
    out = world(scene, orc, st, i, nstep, ids, qpos=qpos)
    out["qfrc_actuator"] = out["qfrc_actuator"] - rows["qfrc_applied"][i]
    out["qfrc_bias"] = out["qfrc_bias"] + generalized_any(orc, scene, np.asarray(rows["xfrc_applied"][i], dtype=np.float64))
    return out


def _stack(rows):
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


_RUNS = {}


def twin_run(name, n, nstep, applied=True):
    """per field the stacked answers of the n twin oracles (applied = False: the force-free scene with the same starts), computed once: read only"""
    key = (name, n, nstep, applied)
    if key not in _RUNS:
        sc = SCENES[name]
        st = sc.states(n)
        ids = D.jac_ids(name) if name in D.JAC_SITES else ()
        if applied:
            rows = twin_rows(sc, n)
            grav, ctrl = twin_reference_inputs(sc, rows, st)
            st = dict(st, ctrl=ctrl)
            _RUNS[key] = _stack([twin_world(sc, P.edited_oracle(sc, dict(gravity=grav), i), st, i, nstep, rows, ids) for i in range(n)])
        else:
            grav = np.broadcast_to(gravity(sc), (n, 3))
            _RUNS[key] = _stack([world(sc, P.edited_oracle(sc, dict(gravity=grav), i), st, i, nstep, ids) for i in range(n)])
    return _RUNS[key]


_SENS = {}


def twin_sensitivity(name, n, nstep, draws=C.DRAWS):
    """[n]: sim_cases.oracle_sensitivity on the twin oracle of every world (the same jitter, generator and seeds), over the float fields, xipos and -- as sim_dyn_cases.error
    measures them -- the seven dynamics vectors"""
    key = (name, n, nstep, draws)
    if key not in _SENS:
        sc = SCENES[name]
        st, base = sc.states(n), twin_run(name, n, nstep)
        rows = twin_rows(sc, n)
        grav, ctrl = twin_reference_inputs(sc, rows, st)
        st = dict(st, ctrl=ctrl)
        sens = np.zeros(n)
        for i in range(n):
            jit = np.random.default_rng([0x6A17, C._name_seed(sc.name), nstep, i])
            q32 = st["qpos"][i].astype(np.float32)
            orc = P.edited_oracle(sc, dict(gravity=grav), i)
            for _ in range(draws):
                up = jit.integers(0, 2, q32.size).astype(bool)
                qj = np.where(up, np.nextafter(q32, np.float32(np.inf)), np.nextafter(q32, np.float32(-np.inf))).astype(np.float64)
                got = twin_world(sc, orc, st, i, nstep, rows, (), qpos=qj)
                for k in S.FLOAT_FIELDS + ("xipos",):
                    if (k == "qpos" and nstep == 0) or not np.asarray(got[k]).size:
                        continue
                    d = np.abs(np.asarray(got[k]) - base[k][i]).max()
                    sens[i] = max(sens[i], d if np.isfinite(d) else np.inf)
                for k in D.VECTORS:
                    sens[i] = max(sens[i], D.error(k, got[k][None], base[k][i][None])[0])
        _SENS[key] = sens
    return _SENS[key]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the closed form (c) on push
_FORM = {}


def form_rows(n=N, chain_only=False):
    """dict(qfrc_applied [n,nv], xfrc_applied [n,nbody,6]) as fp32 values: random forces and torques on every movable body (chain_only: on the chain's bodies alone, and no
    qfrc_applied on the box's dofs -- every loaded dof then carries a gear-1 motor)"""
    key = (n, chain_only)
    if key not in _FORM:
        sc = SCENES["push"]
        nv, nb, names = sc.model.dim("nv"), sc.model.dim("nbody"), sc.model.names["body"]
        x, qf = np.zeros((n, nb, 6)), np.zeros((n, nv))
        for i in range(n):
            r = _rng(sc, i, 3 if chain_only else 2)
            for b in CHAIN_BODIES:
                x[i, names[b]] = np.r_[r.uniform(-2.0, 2.0, 3), r.uniform(-0.5, 0.5, 3)]
            if not chain_only:
                x[i, names["box"]] = np.r_[r.uniform(-0.5, 0.5, 3), r.uniform(-0.5, 0.5, 3)]
            qf[i, :3 if chain_only else nv] = r.uniform(-1.0, 1.0, 3 if chain_only else nv)
        _FORM[key] = dict(qfrc_applied=C.f32(qf), xfrc_applied=C.f32(x))
    return _FORM[key]


def generalized(orc, scene, qf, xf):
    """Q [nv] of the live oracle's configuration: qfrc_applied + sum over the movable bodies of jacp' f + jacr' t with the Jacobians of the centre-of-mass sites (push)"""
    Q = np.array(qf, dtype=np.float64, copy=True)
    for b in MOVABLE:
        jp, jr = orc.jac_site(scene.model.names["site"]["com_" + b])
        row = xf[scene.model.names["body"][b]]
        Q += jp.T @ row[:3] + jr.T @ row[3:]
    return Q


def generalized_any(orc, scene, xf):
    """the body part of Q for a scene without centre-of-mass sites, from what the oracle has: for body b take any site s on b or on a descendant of b; dof d moves b when its
    body is b or an ancestor of b, and then moves the point xipos_b as it moves a point of s's body there: jacp_b[:, d] = jacp_s[:, d] + jacr_s[:, d] x (xipos_b - site_xpos_s),
    jacr_b[:, d] = jacr_s[:, d].  On push it equals generalized() to rounding (tests/test_cpu_sim_applied.py)."""
    m = scene.model
    parent, dof_body, site_body = (np.asarray(m.tables[k]).reshape(-1) for k in ("body_parent", "dof_bodyid", "site_bodyid"))
    nb, nv = m.dim("nbody"), m.dim("nv")

    def ancestors(b):      # b and every body above it, the world excluded
        out = []
        while b > 0:
            out.append(int(b))
            b = parent[b]
        return out

    xipos, sxpos = orc.xipos.reshape(-1, 3), orc.site_xpos.reshape(-1, 3)
    Q = np.zeros(nv)
    for b in range(1, nb):
        if not np.any(xf[b]):
            continue
        s = next(int(i) for i in range(len(site_body)) if b in ancestors(site_body[i]))
        jp, jr = orc.jac_site(s)
        moves = np.array([dof_body[d] in ancestors(b) for d in range(nv)])
        jpb = np.where(moves, jp + np.cross(jr.T, xipos[b] - sxpos[s]).T, 0.0)
        jrb = np.where(moves, jr, 0.0)
        Q += jpb.T @ xf[b, :3] + jrb.T @ xf[b, 3:]
    return Q


def form_run(n=N, qpos=None, world_only=None):
    """the closed form after forward(): per field the stacked expectations of the n worlds (force-free oracle + Q), with Q, nefc and the force-free bias / passive / actuator"""
    key = ("form", n)
    if qpos is None and key in _RUNS:
        return _RUNS[key]
    sc = SCENES["push"]
    st, rows, orc = sc.states(n), form_rows(n), S._oracle(SCENES["push"])
    out = []
    for i in (range(n) if world_only is None else [world_only]):
        w = world(sc, orc, st, i, 0, (), qpos=qpos)
        Q = generalized(orc, sc, rows["qfrc_applied"][i], rows["xfrc_applied"][i])
        M = w["qM"]
        w.update(Q=Q, qfrc_smooth=w["qfrc_smooth"] + Q, qacc_smooth=w["qacc_smooth"] + np.linalg.solve(M, Q))
        w["qacc"] = w["qacc_smooth"] if w["nefc"] == 0 else np.full_like(Q, np.nan)      # with rows the constrained acceleration has no closed form here
        out.append(w)
    res = _stack(out)
    if qpos is None and world_only is None:
        _RUNS[key] = res
    return res


def chain_run(n=N):
    """item 3: step(1) of the oracle with ctrl += Q, Q from forward() at the same state with the chain-only rows (the box's dofs get nothing: its contacts go on elsewhere)"""
    key = ("chain", n)
    if key not in _RUNS:
        sc = SCENES["push"]
        st, rows, orc = sc.states(n), form_rows(n, chain_only=True), S._oracle(SCENES["push"])
        ctrl = np.array(st["ctrl"], dtype=np.float64, copy=True)
        for i in range(n):
            world(sc, orc, st, i, 0)
            Q = generalized(orc, sc, rows["qfrc_applied"][i], rows["xfrc_applied"][i])
            assert not Q[3:].any()      # nothing reaches the box
            for a, (d, gear) in enumerate(motors(sc)):
                ctrl[i, a] += Q[d] / gear
        st = dict(st, ctrl=ctrl)
        _RUNS[key] = _stack([world(sc, orc, st, i, 1) for i in range(n)])
    return _RUNS[key]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# per-world parameters (item 9): two worlds get edited masses and gravity
PARAM_WORLDS = (1, 3)
PARAM_NAMES = ("gravity", "body_mass")


def param_rows(n=N):
    """dict(gravity [n,3], body_mass [n,nbody]): nominal, except in PARAM_WORLDS, where they are the draws of sim_params_cases"""
    sc = SCENES["push"]
    drawn = P.draw(sc, PARAM_NAMES, n)
    rows = {k: np.stack([P.nominal(sc, k)] * n) for k in PARAM_NAMES}
    for w in PARAM_WORLDS:
        for k in PARAM_NAMES:
            rows[k][w] = drawn[k][w]
    return rows


def param_applied(n=N):
    """xfrc_applied = m_b^w a with the world's own masses, as fp32 values"""
    sc = SCENES["push"]
    acc, mass = twin_rows(sc, n)["accel"], param_rows(n)["body_mass"]
    x = np.zeros((n, sc.model.dim("nbody"), 6))
    x[:, :, :3] = mass[:, :, None] * acc[:, None, :]
    x[:, 0] = 0.0
    return C.f32(x)


def param_run(n=N, nstep=4, edited=True):
    """the gravity twin of item 9 on one edited oracle per world (edited = False: every world on the nominal parameters, for the precondition that the edit matters)"""
    key = ("param", n, nstep, edited)
    if key not in _RUNS:
        sc = SCENES["push"]
        st, rows = sc.states(n), (param_rows(n) if edited else {k: np.stack([P.nominal(sc, k)] * n) for k in PARAM_NAMES})
        edit = dict(gravity=rows["gravity"] + twin_rows(sc, n)["accel"], body_mass=rows["body_mass"])
        mass = rows["body_mass"] if edited else np.stack([body_mass(sc)] * n)
        x = np.zeros((n, sc.model.dim("nbody"), 6))
        x[:, :, :3] = mass[:, :, None] * twin_rows(sc, n)["accel"][:, None, :]
        applied = dict(qfrc_applied=np.zeros((n, sc.model.dim("nv"))), xfrc_applied=x)
        _RUNS[key] = _stack([twin_world(sc, P.edited_oracle(sc, edit, i), st, i, nstep, applied, D.jac_ids("push")) for i in range(n)])
    return _RUNS[key]
