"""The dynamics outputs of grx.BatchedSim (tests/test_cpu_sim_dynamics.py, tests/test_gpu_sim_dynamics.py) on top of tests/sim_cases.py: one more scene, the oracle
reader for the ten new fields and their reference-sensitivity measure.  Plain Python and numpy.

anchor .. the arm scene with two more sites: `base` on the world body (its Jacobian is all zeros) and `elbow` on a body without a joint inside link2, which the compiler
          merges into link2 (a site of a merged static child).  Three of the four sites are selected, in an order that differs from their site ids.  Same starts as arm.
pile16 .. the pile of sim_cases with sixteen spheres, every one pressed into the plane, on the default tables: sixteen sites, as many as one launch carries, all selected in
          a scrambled order.  pile17 has one site too many for jac_sites=None.
rows .... the model and the first worlds of the engine matrix's rows-mixed-euler group (engine_matrix_cases.rows_mixed) with a site on the tip of its welded chain: welds, joint
          equalities, friction loss, joint and tendon limits and a contact in every world (nefc > 0: the in-LDS qacc_smooth solve), and qfrc_actuator with both clamps and
          with two actuators on one joint, whose forces add.  Compared like the others, within the bounds the other scenes set.

Error measure.  qM, site_jacp and site_jacr are compared absolutely (entries are O(1)).  The eight force / acceleration vectors are compared per world as
max |got - want| / max(1, max |want|): the arm's qacc reaches 1.5e3, where an absolute 1e-4 would ask more than fp32 holds."""
import numpy as np

import engine_matrix_cases as C
import sim_cases as S

VECTORS = ("qfrc_smooth", "qacc_smooth", "qfrc_constraint", "qacc", "qfrc_bias", "qfrc_passive", "qfrc_actuator")
MATRICES = ("qM", "site_jacp", "site_jacr")
DYNAMICS = ("qM",) + VECTORS + ("site_jacp", "site_jacr")      # the order of sim.OUTPUTS

ANCHOR_XML = S.ARM_XML.replace('<geom name="floor"', '<site name="base" pos="0.1 -0.2 0.3"/>\n    <geom name="floor"').replace(
    '<body name="link3" pos="0.2 0 0">',
    '<body name="bracket" pos="0.1 0.02 0.03"><geom type="sphere" size="0.01" mass="0.05" contype="0" conaffinity="0"/><site name="elbow" pos="0.01 0 0.02"/></body>\n'
    '          <body name="link3" pos="0.2 0 0">')
assert ANCHOR_XML.count('name="base"') == 1 and ANCHOR_XML.count('name="elbow"') == 1



def _pile_xml(k):
    balls = "".join(
        f'<body name="s{i}" pos="{0.1 * (i % 5) - 0.2:.2f} {0.1 * (i // 5) - 0.1:.2f} {S._R}"><joint name="z{i}" type="slide" axis="0 0 1" damping="0.2"/>'
        f'<geom type="sphere" size="{S._R}" mass="{0.05 + 0.01 * i:.2f}" condim="3"/><site name="c{i}" pos="0.01 0 {0.001 * i:.3f}"/></body>' for i in range(k))
    return f'<mujoco><option timestep="0.002"/><worldbody><geom name="floor" type="plane" size="2 2 0.1" condim="3"/>{balls}</worldbody></mujoco>'


def _pilek_states(model, n, seed):
    """every sphere of a pile variant pressed 0.5 .. 2 mm into the plane (the default tables hold them all)"""
    nq, nv, nu, nm = S._dims(model)
    q, v = np.zeros((n, nq)), np.zeros((n, nv))
    for i in range(n):
        r = S._world_rng(seed, i)
        q[i], v[i] = -r.uniform(5e-4, 2e-3, nq), 0.05 * r.standard_normal(nv)
    return dict(qpos=q, qvel=v, ctrl=np.zeros((n, nu)), mocap_pos=np.zeros((n, nm, 3)), mocap_quat=np.zeros((n, nm, 4)))


def _rows_states(model, n, seed):
    """the first n cases of rows-mixed-euler"""
    nm = model.dim("nmocap")
    _, q, v, ctrl = C.rows_mixed("rows-mixed-euler", site=True)
    assert n <= len(q) and q.shape[1] == model.dim("nq")
    return dict(qpos=q[:n], qvel=v[:n], ctrl=ctrl[:n], mocap_pos=np.zeros((n, nm, 3)), mocap_quat=np.zeros((n, nm, 4)))


S._STATES.update(anchor=S._arm_states, pile16=_pilek_states, pile17=_pilek_states, rows=_rows_states)
SCENES = dict(S.SCENES, anchor=S.Scene("anchor", ANCHOR_XML, 15, compile_kwargs=dict(touch_filter=lambda name: True, keep_sites=("ee", "pad", "base", "elbow"))))


class _RowsScene(S.Scene):
    """the rows scene: its MJCF comes from engine_matrix_cases.rows_mixed, which asks the oracle for the welded pose, so it is written on first use and not at import"""
    def __init__(self):
        super().__init__("rows", None, 18)

    @property
    def xml(self):
        if self._xml is None:
            self._xml = C.rows_mixed("rows-mixed-euler", site=True)[0]
        return self._xml

    @xml.setter
    def xml(self, text):
        self._xml = text


SCENES.update(rows=_RowsScene())
SCENES.update(pile16=S.Scene("pile16", _pile_xml(16), 16), pile17=S.Scene("pile17", _pile_xml(17), 17))      # 16 sites: the most one launch carries; 17: one too many
# the selected sites of each scene, in the order of the rows of site_jacp / site_jacr
JAC_SITES = {"arm": ("ee", "pad"), "mocap": ("grip", "pegtip"), "rk4": ("imu", "tip"), "anchor": ("elbow", "base", "ee"), "pile": ("c3", "c0"), "rows": ("tip",),
             "pile16": tuple(f"c{(5 * k) % 16}" for k in range(16))}
BOUND_SCENES = ("arm", "mocap", "rk4", "anchor")      # the scenes whose measured errors set the vector bounds (tests/test_gpu_sim_dynamics.py); rows is held to them
CASES = [(s, k) for s in BOUND_SCENES for k in (0, 1, 4)] + [("rows", 0), ("rows", 1)]


def jac_ids(scene):
    names = SCENES[scene].model.names["site"]
    return tuple(int(names[k]) for k in JAC_SITES[scene])


def _read_dyn(sim, ids):
    nv = sim.nv
    jp, jr = np.zeros((len(ids), 3, nv)), np.zeros((len(ids), 3, nv))
    for r, s in enumerate(ids):
        jp[r], jr[r] = sim.jac_site(s)
    out = {k: getattr(sim, k).copy() for k in VECTORS}
    out.update(qM=sim.M.reshape(nv, nv).copy(), site_jacp=jp, site_jacr=jr)
    return out


def oracle_world(scene, st, i, nstep, ids, qpos=None):
    """sim_cases.oracle_world plus the ten dynamics fields of the same MjData (ids: the selected site ids)"""
    out = S.oracle_world(scene, st, i, nstep, qpos=qpos)      # leaves the live oracle at the answer
    out.update(_read_dyn(S._oracle(scene), ids))
    return out


_RUNS = {}


def oracle_run(name, n, nstep):
    """per field the stacked answers of the n worlds (the fields of sim_cases.oracle_run and the ten new ones), computed once per (scene, n, nstep): read only"""
    key = (name, n, nstep)
    if key not in _RUNS:
        sc, ids = SCENES[name], jac_ids(name)
        rows = [oracle_world(sc, sc.states(n), i, nstep, ids) for i in range(n)]
        _RUNS[key] = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
    return _RUNS[key]


def error(field, got, want):
    """[n]: per world the compared error of a dynamics field -- absolute for the matrices, normalised by max(1, |that world's reference row|_inf) for the vectors"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    n = want.shape[0]
    d = np.abs(got.reshape(n, -1) - want.reshape(n, -1)).max(axis=1) if want.size else np.zeros(n)
    d = np.where(np.isfinite(d), d, np.inf)
    if field in MATRICES:
        return d
    return d / np.maximum(1.0, np.abs(want.reshape(n, -1)).max(axis=1))


_SENS = {}


def oracle_sensitivity(name, n, nstep, draws=C.DRAWS):
    """{field: [n]}: the largest error() of the oracle's own answer against itself over `draws` re-runs with the one-fp32-ulp qpos jitter of sim_cases.oracle_sensitivity
    (the same generator and seeds, so the same jittered starts)"""
    key = (name, n, nstep, draws)
    if key not in _SENS:
        sc, ids = SCENES[name], jac_ids(name)
        st, base = sc.states(n), oracle_run(name, n, nstep)
        sens = {k: np.zeros(n) for k in DYNAMICS}
        for i in range(n):
            jit = np.random.default_rng([0x6A17, C._name_seed(sc.name), nstep, i])
            q32 = st["qpos"][i].astype(np.float32)
            for _ in range(draws):
                up = jit.integers(0, 2, q32.size).astype(bool)
                qj = np.where(up, np.nextafter(q32, np.float32(np.inf)), np.nextafter(q32, np.float32(-np.inf))).astype(np.float64)
                got = oracle_world(sc, st, i, nstep, ids, qpos=qj)
                for k in DYNAMICS:
                    sens[k][i] = max(sens[k][i], error(k, got[k][None], base[k][i][None])[0])
        _SENS[key] = sens
    return _SENS[key]
