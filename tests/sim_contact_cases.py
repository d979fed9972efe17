"""The contact outputs of grx.BatchedSim (tests/test_cpu_sim_contacts.py, tests/test_gpu_sim_contacts.py) on top of tests/sim_cases.py: one more scene, the oracle reader
for the seven members of the contact list, a numpy restatement of the force decode, the matching rule and the reference-sensitivity measure.  Plain Python and numpy.

cones ... a condim-1 plane; a hinge with friction loss started beyond its upper limit (one friction row and one limit row in front of the contacts' rows); a condim-1
          sphere on a vertical slide (one contact, one row); a free condim-4 box (four contacts, six rows each); a free condim-6 sphere (one contact, ten rows).  Each body
          is pressed 0.3 .. 2 mm into the plane.  Even worlds slide and spin; odd worlds have no linear velocity and only spin, with torsional / rolling friction raised to
          0.2 / 0.05: a sliding contact puts its whole load on one edge of the pyramid, where the torsional and rolling components are exact zeros.

FORCE DECODE (mj_contactForce, pyramidal cone).  With f the contact's rows of efc_force and mu the pair's friction row: dim 1: force[0] = f[0]; otherwise force[0] = sum f
and force[k] = mu[k - 1] (f[2 (k - 1)] - f[2 (k - 1) + 1]) for 1 <= k < dim; components at index dim and above are 0; a contact without rows has zero force.

FRAME.  The oracle keeps the normal; the two tangents are those of the rule both engines share (MuJoCo's mju_makeFrame: y = e_y unless |n_y| >= 0.5, then e_z;
orthogonalised against the normal; z = n x y), restated here in fp64.

MATCHING.  The device lists its contacts in the engine's order, the oracle in its own.  Per world they are paired by (geom1, geom2) and within a pair greedily by nearest
pos; the counts must be equal and every contact is matched: none of a compared world is left out.

Error measure.  dist / pos / frame absolutely; force per world as max |got - want| / max(1, max |want|) over the world's contacts."""
import numpy as np

import engine_matrix_cases as C
import sim_cases as S

CONTACTS = ("contact_geom", "contact_dim", "contact_efc_address", "contact_dist", "contact_pos", "contact_frame", "contact_force")
INTS = ("contact_geom", "contact_dim", "contact_efc_address")
GEOMETRIC = ("contact_dist", "contact_pos", "contact_frame")
FILL = dict(contact_geom=-1, contact_dim=0, contact_efc_address=-1, contact_dist=0.0, contact_pos=0.0, contact_frame=0.0, contact_force=0.0)

CONES_XML = """<mujoco>
  <compiler angle="radian"/>
  <option timestep="0.002"/>
  <worldbody>
    <geom name="floor" type="plane" size="2 2 0.1" condim="1" friction="1 0.005 0.0001"/>
    <body name="lever" pos="-0.4 0 0.3">
      <joint name="lj" type="hinge" axis="0 1 0" limited="true" range="-0.5 0.5" damping="0.1" frictionloss="0.05" armature="0.01"/>
      <geom type="capsule" fromto="0 0 0 0.2 0 0" size="0.02" mass="0.3" contype="0" conaffinity="0"/>
    </body>
    <body name="ball1" pos="0 0 0.03">
      <joint name="z1" type="slide" axis="0 0 1" damping="0.2"/>
      <geom name="g1" type="sphere" size="0.03" mass="0.1" condim="1"/>
    </body>
    <body name="puck" pos="0.3 0 0.02">
      <freejoint name="pj"/>
      <geom name="g4" type="box" size="0.05 0.04 0.02" mass="0.2" condim="4" friction="0.8 0.2 0.0001"/>
    </body>
    <body name="ball6" pos="0 0.3 0.04">
      <freejoint name="bj"/>
      <geom name="g6" type="sphere" size="0.04" mass="0.15" condim="6" friction="0.7 0.2 0.05"/>
    </body>
  </worldbody>
</mujoco>"""


def _cones_states(model, n, seed):
    nq, nv, nu, nm = S._dims(model)
    q, v = np.zeros((n, nq)), np.zeros((n, nv))
    for i in range(n):
        r = S._world_rng(seed, i)
        slide = 0.0 if i % 2 else 1.0      # odd worlds only spin
        q[i, 0] = 0.5 + r.uniform(1e-3, 5e-3)      # the lever beyond its upper limit
        v[i, 0] = 0.5 * r.standard_normal()
        q[i, 1], v[i, 1] = -r.uniform(5e-4, 2e-3), 0.05 * r.standard_normal()
        q[i, 2:5] = [0.3 + 0.05 * r.standard_normal(), 0.05 * r.standard_normal(), 0.02 - r.uniform(3e-4, 2e-3)]
        q[i, 5:9] = C.axis_angle([0, 0, 1], r.uniform(-np.pi, np.pi))
        v[i, 2:8] = np.r_[slide * 0.2 * r.standard_normal(2), 0.0, 0.0, 0.0, 2.0 * r.standard_normal()]
        q[i, 9:12] = [0.05 * r.standard_normal(), 0.3 + 0.05 * r.standard_normal(), 0.04 - r.uniform(3e-4, 2e-3)]
        q[i, 12:16] = C._unit(r, 4)
        v[i, 8:14] = np.r_[slide * 0.2 * r.standard_normal(2), 0.0, 1.0 * r.standard_normal(3)]
    return dict(qpos=q, qvel=v, ctrl=np.zeros((n, nu)), mocap_pos=np.zeros((n, nm, 3)), mocap_quat=np.zeros((n, nm, 4)))


S._STATES.update(cones=_cones_states)
SCENES = dict(arm=S.SCENES["arm"], mocap=S.SCENES["mocap"], pile=S.SCENES["pile"], cones=S.Scene("cones", CONES_XML, 19))
N = S.N_WORLDS
CASES = [(s, k, N) for s in ("arm", "mocap", "cones") for k in (0, 1, 4)] + [("arm", 1, 13)]      # item 1 of the GPU file; the table of measured errors has one row each
PILE_CASES = [("pile", 1, N), ("pile", 4, N)]
FREE_BODIES = {"arm": (("boxg", 4),), "cones": (("g4", 2), ("g6", 8))}      # free bodies that touch only the plane: (geom, first translational dof)


def make_frame(normal):
    """[9]: the normal and the two tangents of mju_makeFrame, fp64"""
    x = np.asarray(normal, dtype=np.float64)
    y = np.array([0.0, 1.0, 0.0]) if -0.5 < x[1] < 0.5 else np.array([0.0, 0.0, 1.0])
    y = y - (x @ y) * x
    y = y / np.linalg.norm(y)
    return np.r_[x, y, np.cross(x, y)]


def decode_force(f, address, dim, mu):
    """[6]: mj_contactForce of one contact for the pyramidal cone (module docstring)"""
    w = np.zeros(6)
    if address < 0:
        return w
    if dim == 1:
        w[0] = f[address]
        return w
    rows = f[address:address + 2 * (dim - 1)]
    w[0] = rows.sum()
    for k in range(1, dim):
        w[k] = mu[k - 1] * (rows[2 * (k - 1)] - rows[2 * (k - 1) + 1])
    return w


def rows_of(dim, address):
    """constraint rows of a contact"""
    return 0 if address < 0 else (1 if dim == 1 else 2 * (dim - 1))


def pair_of(model, g1, g2):
    a, b = (np.asarray(model.tables[k]).reshape(-1) for k in ("pair_geom1", "pair_geom2"))
    hit = np.nonzero((a == g1) & (b == g2))[0]
    assert len(hit) == 1, (g1, g2, hit)
    return int(hit[0])


def read_contacts(scene, sim, friction=None):
    """the contact list of the live oracle, in ITS order: one array per member of CONTACTS plus nefc and qfrc_constraint.
    friction: the [npair, 5] table the forces are decoded with (None: the model's, as fp32 holds it -- what the device reads)"""
    mu = C.f32(np.asarray(scene.model.tables["pair_friction"]).reshape(-1, 5)) if friction is None else np.asarray(friction, dtype=np.float64).reshape(-1, 5)
    con, f = sim.contacts(), sim.efc("force")
    assert len(con) == sim.ncon, "the oracle's list is longer than its reader holds"
    n = len(con)
    out = dict(contact_geom=np.zeros((n, 2), dtype=np.int64), contact_dim=np.zeros(n, dtype=np.int64), contact_efc_address=np.zeros(n, dtype=np.int64),
               contact_dist=np.zeros(n), contact_pos=np.zeros((n, 3)), contact_frame=np.zeros((n, 9)), contact_force=np.zeros((n, 6)))
    for k, c in enumerate(con):
        g1, g2, dim, adr = int(c[7]), int(c[8]), int(c[9]), int(c[10])
        out["contact_geom"][k], out["contact_dim"][k], out["contact_efc_address"][k] = (g1, g2), dim, adr
        out["contact_dist"][k], out["contact_pos"][k], out["contact_frame"][k] = c[0], c[1:4], make_frame(c[4:7])
        out["contact_force"][k] = decode_force(f, adr, dim, mu[pair_of(scene.model, g1, g2)])
    out["nefc"] = int(sim.nefc)
    out["qfrc_constraint"] = sim.qfrc_constraint.copy()
    return out


def oracle_world(scene, st, i, nstep, qpos=None, friction=None):
    S.oracle_world(scene, st, i, nstep, qpos=qpos)      # leaves the live oracle at the answer
    return read_contacts(scene, S._oracle(scene), friction)


FRICTION_WORLDS = (1, 3)      # the per-world parameter case of the GPU file: pair_friction doubled in these worlds of cones
FRICTION_CASES = [("cones", 0, N), ("cones", 4, N)]


def friction_rows(n=N):
    """dict(pair_friction [n, npair, 5]): the cones model's table as fp32 holds it, doubled in FRICTION_WORLDS"""
    nominal = C.f32(np.asarray(SCENES["cones"].model.tables["pair_friction"]).reshape(-1, 5))
    return dict(pair_friction=np.stack([nominal * (2.0 if w in FRICTION_WORLDS else 1.0) for w in range(n)]))


def _world(name, n, i, nstep, edit, qpos=None):
    """world i of a case on the scene's oracle; edit: on an oracle whose pair_friction table holds the world's row of friction_rows (the same in-place edit the device
    commits), decoded with that row"""
    sc = SCENES[name]
    if not edit:
        return oracle_world(sc, sc.states(n), i, nstep, qpos=qpos)
    import sim_params_cases as P

    rows = friction_rows(n)
    with P.standing_in(sc, P.edited_oracle(sc, rows, i)):
        return oracle_world(sc, sc.states(n), i, nstep, qpos=qpos, friction=rows["pair_friction"][i])


_RUNS = {}


def oracle_run(name, n, nstep, edit=False):
    """[n] lists of read_contacts, computed once per (scene, n, nstep, edit): read only"""
    key = (name, n, nstep, edit)
    if key not in _RUNS:
        _RUNS[key] = [_world(name, n, i, nstep, edit) for i in range(n)]
    return _RUNS[key]


def match(dev_geom, dev_pos, want):
    """index array p with device contact p[k] <-> oracle contact k of one world: by (geom1, geom2), within a pair greedily by nearest pos.  Raises when the counts or the
    pairs differ: every contact of a compared world is matched"""
    dev_geom, dev_pos = np.asarray(dev_geom), np.asarray(dev_pos, dtype=np.float64)
    n = len(want["contact_dim"])
    assert len(dev_geom) == n, f"the device lists {len(dev_geom)} contacts, the oracle {n}"
    free, perm = list(range(n)), np.full(n, -1)
    for k in range(n):
        cand = [j for j in free if tuple(dev_geom[j]) == tuple(want["contact_geom"][k])]
        assert cand, f"oracle contact {k} of geoms {tuple(want['contact_geom'][k])} has no device contact left; the device lists {dev_geom.tolist()}"
        j = min(cand, key=lambda j: np.abs(dev_pos[j] - want["contact_pos"][k]).max())
        perm[k] = j
        free.remove(j)
    return perm


def force_error(got, want):
    """normalised error of one world's forces [n, 6]"""
    want = np.asarray(want, dtype=np.float64)
    if not want.size:
        return 0.0
    d = np.abs(np.asarray(got, dtype=np.float64) - want).max()
    return float(d / max(1.0, np.abs(want).max())) if np.isfinite(d) else np.inf


def force_bound():
    """the asserted bound of contact_force: the smallest power of ten >= 4 x the worst normalised error measured on the MI355X over CASES (tests/golden/sim_contact_errors.json,
    one row per scene / nstep / world count; the margin of 4 covers summation-order changes between compiler versions -- the rule of sim_dynamics_errors.json)"""
    import json
    import math
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim_contact_errors.json")) as fh:
        table = json.load(fh)["worst_error"]
    worst = max(table[f"{s}/{k}/{n}"]["contact_force"] for s, k, n in CASES)
    return 10.0 ** math.ceil(math.log10(4.0 * worst))


_SENS = {}


def oracle_sensitivity(name, n, nstep, draws=C.DRAWS, edit=False):
    """dict(same [n] bool, geometric [n], force [n]): over `draws` re-runs with the one-fp32-ulp qpos jitter of sim_cases.oracle_sensitivity (the same generator and seeds) --
    whether the contact set (geoms, dim, efc_address, in the oracle's order) stayed what it was, the largest absolute change of dist / pos / frame, the largest force_error"""
    key = (name, n, nstep, draws, edit)
    if key not in _SENS:
        sc = SCENES[name]
        st, base = sc.states(n), oracle_run(name, n, nstep, edit)
        same, geo, frc = np.ones(n, dtype=bool), np.zeros(n), np.zeros(n)
        for i in range(n):
            jit = np.random.default_rng([0x6A17, C._name_seed(sc.name), nstep, i])
            q32 = st["qpos"][i].astype(np.float32)
            for _ in range(draws):
                up = jit.integers(0, 2, q32.size).astype(bool)
                qj = np.where(up, np.nextafter(q32, np.float32(np.inf)), np.nextafter(q32, np.float32(-np.inf))).astype(np.float64)
                got = _world(name, n, i, nstep, edit, qpos=qj)
                if any(got[k].shape != base[i][k].shape or (got[k] != base[i][k]).any() for k in INTS):
                    same[i] = False
                    break
                for k in GEOMETRIC:
                    if got[k].size:
                        geo[i] = max(geo[i], np.abs(got[k] - base[i][k]).max())
                frc[i] = max(frc[i], force_error(got["contact_force"], base[i]["contact_force"]))
        _SENS[key] = dict(same=same, geometric=geo, force=frc)
    return _SENS[key]
