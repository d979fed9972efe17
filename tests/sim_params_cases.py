"""Per-world model parameters of grx.BatchedSim (tests/test_cpu_sim_params.py, tests/test_gpu_sim_params.py): the scenes, the drawn parameter rows and the edited oracle.

Scenes: arm, rk4 and pile of tests/sim_cases.py, and armv -- the arm with frictionloss on two hinges and a stiffness / springref on a third, which the arm has not.

Rows: draw(scene, names, n) gives every world its own row of each named table from a seeded generator, rounded to fp32: factors in [0.5, 2] for masses, inertias, damping,
armature, frictionloss, stiffness, gear, gains and friction; gravity rotated by up to 30 degrees about a random axis and scaled by +-30 %; ranges scaled end by end.

Reference: one OracleSim per world with the same fp32 values written through OracleSim.model_table into the named tables (gravity: words 1..3 of `opt`) -- in-place MjModel
edits without mj_setConst, the operational definition of the feature.  The readers are those of sim_cases / sim_dyn_cases: the edited oracle stands in for the scene's own
while they run."""
import contextlib

import numpy as np

import engine_matrix_cases as C
import sim_cases as S
import sim_dyn_cases as D

N = S.N_WORLDS
ALL = ("gravity", "body_mass", "body_inertia", "dof_damping", "dof_armature", "dof_frictionloss", "jnt_stiffness", "jnt_springref", "jnt_range", "act_gear", "act_gainprm",
       "act_biasprm", "act_ctrlrange", "act_forcerange", "pair_friction", "pair_solref", "pair_solimp")
GROUPS = {"inertial": ("body_mass", "body_inertia"), "dof": ("dof_damping", "dof_armature", "dof_frictionloss"), "joint": ("jnt_stiffness", "jnt_springref", "jnt_range"),
          "actuator": ("act_gear", "act_gainprm", "act_biasprm", "act_ctrlrange", "act_forcerange"), "pair": ("pair_friction", "pair_solref", "pair_solimp"),
          "gravity": ("gravity",), "all": ALL}

ARMV_XML = (S.ARM_XML.replace('range="-1.5 1.5" damping="0.3"', 'range="-1.5 1.5" damping="0.3" frictionloss="0.05"')
            .replace('range="-0.4 1.8" damping="0.2"', 'range="-0.4 1.8" damping="0.2" frictionloss="0.03"')
            .replace('range="-1 1" damping="0.1"', 'range="-1 1" damping="0.1" stiffness="2" springref="0.3"'))
assert ARMV_XML.count("frictionloss") == 2 and ARMV_XML.count("springref") == 1
S._STATES.setdefault("armv", S._arm_states)      # the variant starts where the arm starts
SCENES = dict(S.SCENES, armv=S.Scene("armv", ARMV_XML, 11, compile_kwargs=dict(touch_filter=lambda name: True, keep_sites=("ee", "pad"))))
D.SCENES.setdefault("armv", SCENES["armv"])
D.JAC_SITES.setdefault("armv", ("ee", "pad"))
# a group is run on the scenes that have something of it: rk4 has no candidate pair, the pile no actuator
GROUP_SCENES = {"inertial": ("armv", "rk4"), "dof": ("armv", "rk4"), "joint": ("armv", "rk4"), "actuator": ("armv", "rk4"), "pair": ("armv",), "gravity": ("armv", "rk4"),
                "all": ("armv", "rk4")}
GROUP_CASES = [(g, s) for g in GROUPS for s in GROUP_SCENES[g]]
PILE_PARAMS = ("gravity", "pair_friction")      # the overflow re-run with per-world parameters
STEPS = (1, 4, 0)     # step(1), step(4), forward()


def nominal(scene, name):
    """the model's own fp32 values of a parameter, in the shape of one world's row of sim.params.<name>"""
    m = scene.model
    if name == "gravity":
        return C.f32(np.asarray(m.tables["opt"], dtype=np.float64).reshape(-1)[1:4])
    a = np.asarray(m.tables[name], dtype=np.float64)
    while a.ndim > 1 and a.shape[-1] == 1:
        a = a[..., 0]
    return C.f32(a)


def _draw_one(name, nom, r, dt):
    f = lambda shape=(): r.uniform(0.5, 2.0, shape)
    a = nom.copy()
    if name == "gravity":
        return _rotate(C._unit(r, 3), r.uniform(-np.pi / 6, np.pi / 6), nom) * r.uniform(0.7, 1.3)
    if name in ("body_mass", "dof_damping", "dof_armature", "dof_frictionloss", "jnt_stiffness", "act_gear"):
        return a * f(a.shape)
    if name == "body_inertia":
        return a * f((a.shape[0], 1))      # one factor per body: the inertia stays that of a body
    if name == "jnt_springref":
        return a + r.uniform(-0.2, 0.2, a.shape)
    if name in ("jnt_range", "act_ctrlrange", "act_forcerange"):
        return a * r.uniform(0.7, 1.3, a.shape)      # every range of these scenes has lower end < 0 < upper end, or is 0 0 (not limited)
    if name in ("act_gainprm", "act_biasprm", "pair_friction"):
        return a * f((a.shape[0], 1))
    if name == "pair_solref":
        a[:, 0] = np.maximum(a[:, 0], 2.0 * dt) * r.uniform(1.0, 2.0, a.shape[0])      # a time constant stays above two time steps
        a[:, 1] *= r.uniform(0.7, 1.3, a.shape[0])
        return a
    if name == "pair_solimp":
        a[:, 0] *= r.uniform(0.9, 1.0, a.shape[0])
        a[:, 1] = 1.0 - (1.0 - a[:, 1]) * r.uniform(0.5, 2.0, a.shape[0])
        a[:, 2] *= r.uniform(0.5, 2.0, a.shape[0])
        return a
    raise KeyError(name)


def _rotate(axis, angle, v):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    return v * np.cos(angle) + np.cross(axis, v) * np.sin(angle) + axis * np.dot(axis, v) * (1.0 - np.cos(angle))


_DRAWS = {}
# draws that were replaced (scene, table, world) -> which redraw: the first draw left the world within a hundred bounds of the nominal model in every compared field
# (tests/test_cpu_sim_params.py test_every_drawn_world_differs_from_the_nominal_model) -- a spring drawn next to its rest position, a gravity change along the floor's normal only
REDRAWN = {("rk4", "jnt_stiffness", 4): 1, ("rk4", "jnt_springref", 4): 1, ("rk4", "jnt_range", 4): 1, ("armv", "gravity", 4): 1}


def draw(scene, names, n=N):
    """{name: [n, ...] fp32-valued float64 rows}; world i's row of a table is the same whatever else is named and whatever n is"""
    out = {}
    for name in names:
        key = (scene.name, name, n)
        if key not in _DRAWS:
            nom = nominal(scene, name)
            seed = lambda i: [0x9A7A, scene.seed, ALL.index(name), i] + ([REDRAWN[scene.name, name, i]] if (scene.name, name, i) in REDRAWN else [])
            rows = [_draw_one(name, nom, np.random.default_rng(seed(i)), scene.model.opt("timestep")) for i in range(n)]
            _DRAWS[key] = C.f32(np.stack(rows))
        out[name] = _DRAWS[key]
    return out


def load_params(sim, rows, worlds=None):
    """write the rows into sim.params (worlds: only those)"""
    import torch

    for name, a in rows.items():
        dst = getattr(sim.params, name)
        src = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(dst.shape).to(dst.device)
        if worlds is None:
            dst.copy_(src)
        else:
            dst[list(worlds)] = src[list(worlds)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the edited oracle
def edited_oracle(scene, rows, i):
    """a fresh OracleSim of the scene with world i's rows written into its model"""
    from oracle.oracle_sim import OracleSim

    sim = OracleSim(scene.model)
    for name, a in rows.items():
        v = np.asarray(a[i], dtype=np.float64).reshape(-1)
        if name == "gravity":
            sim.model_table("opt", 4)[1:4] = v
        elif v.size:
            sim.model_table(name, v.size)[:] = v
    return sim


@contextlib.contextmanager
def standing_in(scene, sim):
    """sim_cases / sim_dyn_cases read the oracle of a scene through sim_cases._ORACLES: let `sim` be it for a while"""
    old = S._ORACLES.get(scene.name)
    S._ORACLES[scene.name] = sim
    try:
        yield
    finally:
        if old is None:
            del S._ORACLES[scene.name]
        else:
            S._ORACLES[scene.name] = old


_RUNS = {}


def oracle_run(scene, rows_key, rows, n, nstep, dyn_ids=None):
    """per field the stacked answers of the n edited worlds after step(nstep) (0: forward()); rows_key names the rows for the cache.  dyn_ids: also the dynamics fields"""
    key = (scene.name, rows_key, n, nstep, dyn_ids)
    if key not in _RUNS:
        st, out = scene.states(n), []
        for i in range(n):
            with standing_in(scene, edited_oracle(scene, rows, i)):
                out.append(S.oracle_world(scene, st, i, nstep) if dyn_ids is None else D.oracle_world(scene, st, i, nstep, dyn_ids))
        _RUNS[key] = {k: np.stack([np.asarray(r[k]) for r in out]) for k in out[0]}
    return _RUNS[key]


_SENS = {}
DYN_PARAMS = ("body_mass", "dof_armature", "gravity")      # the dynamics-block case: its own rows key ("dynamics"), its own preconditions
DYN_FIELDS = ("qM", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "qacc")


def oracle_sensitivity(scene, rows_key, rows, n, nstep, draws=C.DRAWS, dyn_fields=("qacc",)):
    """[n]: sim_cases.oracle_sensitivity on the EDITED oracle of every world -- the largest change of a compared float field over `draws` re-runs in which every qpos component
    of the start moves to a neighbouring fp32 value (the same generator and seeds) -- and, as sim_dyn_cases.oracle_sensitivity measures them (sim_dyn_cases.error), of the
    dynamics fields the GPU test compares: every figure is held to the same SENS_MAX"""
    key = (scene.name, rows_key, n, nstep, draws, dyn_fields)
    if key not in _SENS:
        st, base = scene.states(n), oracle_run(scene, rows_key, rows, n, nstep, ())
        sens = np.zeros(n)
        for i in range(n):
            jit = np.random.default_rng([0x6A17, C._name_seed(scene.name), nstep, i])
            q32 = st["qpos"][i].astype(np.float32)
            with standing_in(scene, edited_oracle(scene, rows, i)):
                for _ in range(draws):
                    up = jit.integers(0, 2, q32.size).astype(bool)
                    qj = np.where(up, np.nextafter(q32, np.float32(np.inf)), np.nextafter(q32, np.float32(-np.inf))).astype(np.float64)
                    got = D.oracle_world(scene, st, i, nstep, (), qpos=qj)
                    for k in S.FLOAT_FIELDS:
                        if k == "qpos" and nstep == 0:
                            continue
                        d = np.abs(np.asarray(got[k]) - base[k][i]).max() if np.asarray(got[k]).size else 0.0
                        sens[i] = max(sens[i], d if np.isfinite(d) else np.inf)
                    for k in dyn_fields:
                        sens[i] = max(sens[i], D.error(k, got[k][None], base[k][i][None])[0])
        _SENS[key] = sens
    return _SENS[key]


COMPARED = S.FLOAT_FIELDS + ("qacc",)      # the fields of sim_cases, within C.BOUND, and the acceleration of the same pass, within its bound of tests/test_gpu_sim_dynamics.py:
# forward() moves none of the kinematic fields whatever the parameters are, and one substep moves them by an acceleration times dt squared


def distance_from_nominal(scene, run, n, nstep, dyn_fields=("qacc",), dyn_bounds=None):
    """[n]: how far each edited world's answer is from the NOMINAL oracle's, as the largest ratio of a compared field's difference to that field's bound x 100 (a world
    with a ratio above 1 differs by more than a hundred bounds in some compared field).  run: oracle_run(..., dyn_ids=())"""
    with standing_in(scene, S._oracle(scene)):
        rows = [D.oracle_world(scene, scene.states(n), i, nstep, ()) for i in range(n)]
    base = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
    ratio = np.zeros(n)
    for k in S.FLOAT_FIELDS + tuple(dyn_fields):
        if not np.asarray(base[k]).size or (k == "qpos" and nstep == 0):
            continue
        if k in dyn_fields:      # dyn_bounds: {field: bound} of tests/test_gpu_sim_dynamics.py for fields other than qacc
            d, bound = D.error(k, run[k], base[k]), (qacc_bound() if k == "qacc" else dyn_bounds[k])
        else:
            d, bound = np.abs(np.asarray(run[k]) - np.asarray(base[k])).reshape(n, -1).max(axis=1), C.BOUND
        ratio = np.maximum(ratio, d / (100.0 * bound))
    return ratio


def vector_bound(field):
    """the bound of tests/test_gpu_sim_dynamics.py for a vector field: the smallest power of ten >= 4 x the worst figure of tests/golden/sim_dynamics_errors.json over its bound cases"""
    import json
    import math
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim_dynamics_errors.json")) as fh:
        table = json.load(fh)["worst_error"]
    cases = [f"{s}/{k}/{N}" for s, k in D.CASES if s in D.BOUND_SCENES] + ["arm/1/13"]
    return 10.0 ** math.ceil(math.log10(4.0 * max(table[c][field] for c in cases)))


def qacc_bound():
    return vector_bound("qacc")


def dyn_bounds():
    """{field: bound} of the dynamics-block case: C.BOUND absolute for qM, the vector bounds for the rest (tests/test_gpu_sim_dynamics.py)"""
    return {k: (C.BOUND if k in D.MATRICES else vector_bound(k)) for k in DYN_FIELDS}
