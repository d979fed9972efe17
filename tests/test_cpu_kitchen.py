"""FrankaKitchen-v1 on the CPU side: registry / spec logic against the reference's source text, the C noise sampler against numpy (symbol check only
without a GPU: the sampler is host code in the HIP library), and the DEVICE ENGINE SOURCE (lane emulator) against the oracle's golden fixtures."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
REF = "/root/reference/gymnasium_robotics/envs"


@pytest.fixture(scope="module")
def model():
    from gymnasium_robotics_amd.envs.kitchen_spec import load_kitchen_model

    return load_kitchen_model()


def test_registry_model_and_constants(model):
    import gymnasium_robotics_amd as grx
    from gymnasium_robotics_amd.envs import kitchen_spec as ks

    assert grx.env_family("FrankaKitchen-v1") == "kitchen" and "FrankaKitchen-v1" in grx.registered_env_ids()
    # SURVEY.md 8(a) cfg 5a: 30 / 29 / 9; five joint equalities (oven_asset.xml:40-46); condim-6 finger pads; no pair left unsupported
    assert (model.dim("nq"), model.dim("nv"), model.dim("nu")) == (30, 29, 9) and len(model.tables["jeq_eq"]) == 5 and model.info["unsupported_pairs"] == 0
    assert int(np.max(model.tables["pair_condim"])) == 6
    assert int(np.round(1.0 / (model.opt("timestep") * ks.FRAME_SKIP))) == 12                 # the render_fps assert of kitchen_env.py:312-314
    assert ks.OBS_DIM == model.dim("nq") + model.dim("nv") and ks.task_mask(ks.TASKS) == 127
    with pytest.raises(ValueError, match="cannot be found"):
        ks.task_mask(["kettle", "toaster"])
    # object qpos slices and goals line up with the compiled joint order (knob pairs, light, slide, hinges, microwave, free kettle)
    J, qadr = model.names["joint"], np.asarray(model.tables["jnt_qposadr"]).ravel()
    assert [int(qadr[J[n]]) for n in ("knob_Joint_2", "bottom_left_burner", "knob_Joint_4", "top_left_burner", "light_switch", "light_joint", "slide_cabinet",
                                      "left_hinge_cabinet", "right_hinge_cabinet", "microwave", "kettle")] == [11, 12, 15, 16, 17, 18, 19, 20, 21, 22, 23]
    cfg = ks.franka_config(model)
    assert cfg["pos_bound"].shape == (29, 2) and np.allclose(cfg["pos_bound"][3], [-3.1, 0.0]) and np.allclose(cfg["vel_bound"][:9], [-10, 10])
    ns = ks.noise_scales(model, 0.01, 0.0005)
    assert ns.shape == (59,) and np.allclose(ns[:18], 0.001) and np.isclose(ns[18], 0.0005 * 0.1) and np.isclose(ns[19], 0.0005 * 0.005)   # pos_noise_amp[8:] starts at the second finger


def _reference_constants():
    """OBS_ELEMENT_INDICES / OBS_ELEMENT_GOALS / BONUS_THRESH and the 30-element init_qpos literal, evaluated from kitchen_env.py's source text (the module
    itself needs MuJoCo).  Where the reference tree is absent: the values stored from it in tests/golden/ref_kitchen_constants.json (GRX_REF_RECORD=1 writes it)."""
    import ast
    import json

    stored = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kitchen_constants.json")
    if not os.path.isdir(REF):
        with open(stored) as f:
            return json.load(f)
    src = open(os.path.join(REF, "franka_kitchen", "kitchen_env.py")).read()
    tree = ast.parse(src)
    ns = {"np": np}
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") in ("OBS_ELEMENT_INDICES", "OBS_ELEMENT_GOALS", "BONUS_THRESH"):
            exec(compile(ast.Module([node], []), "kitchen_env.py", "exec"), ns)
    lit = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "attr", "") == "array" and n.args and isinstance(n.args[0], ast.List)
           and len(n.args[0].elts) == 30]
    assert len(lit) == 1
    c = {"BONUS_THRESH": ns["BONUS_THRESH"], "OBS_ELEMENT_GOALS": {t: np.asarray(v).tolist() for t, v in ns["OBS_ELEMENT_GOALS"].items()},
         "OBS_ELEMENT_INDICES": {t: np.asarray(v).tolist() for t, v in ns["OBS_ELEMENT_INDICES"].items()}, "INIT_QPOS": ast.literal_eval(lit[0].args[0])}
    if os.environ.get("GRX_REF_RECORD") == "1":
        with open(stored, "w") as f:
            json.dump(c, f, indent=1)
    return c


def test_constants_equal_the_reference_source():
    """INIT_QPOS / task indices / goals / BONUS_THRESH are literals of kitchen_env.py."""
    from gymnasium_robotics_amd.envs import kitchen_spec as ks

    ns = _reference_constants()
    assert ns["BONUS_THRESH"] == ks.BONUS_THRESH and list(ns["OBS_ELEMENT_GOALS"]) == ks.TASKS
    for t in ks.TASKS:
        assert np.array_equal(ns["OBS_ELEMENT_INDICES"][t], ks.OBS_ELEMENT_INDICES[t]) and np.array_equal(ns["OBS_ELEMENT_GOALS"][t], ks.OBS_ELEMENT_GOALS[t])
    assert np.array_equal(np.array(ns["INIT_QPOS"]), ks.INIT_QPOS)


def test_task_bookkeeping_masks():
    from gymnasium_robotics_amd.envs import kitchen_spec as ks

    q = np.tile(ks.INIT_QPOS, (3, 1))
    q[1, 22] = -0.75                      # microwave at its goal
    q[2, 19], q[2, 17:19] = 0.37, [-0.69, -0.05]
    m = ks.completed_mask(q)
    assert list(m) == [0, 1 << ks.TASKS.index("microwave"), (1 << ks.TASKS.index("slide cabinet")) | (1 << ks.TASKS.index("light switch"))]


def test_emulated_kernel_matches_golden(model):
    """Teacher-forced env.step() of the engine source (fp32, emulated lanes) against every fourth of the 248 oracle snapshots: robot-only motion,
    arm-vs-scene contacts (condim 6 finger pads, hull pairs), the dropping kettle, the five joint equalities in every substep, the recorded noise."""
    from emu_sim import EmuSim

    from gymnasium_robotics_amd.envs.kitchen_spec import make_kitchen_task

    g = np.load(os.path.join(GOLDEN, "kitchen_teacher.npz"))
    emu = EmuSim(model, make_kitchen_task(model, 0.01, 0.0005))
    errs = []
    for i in range(0, g["obs"].shape[0], 4):
        emu.qpos[:], emu.qvel[:], emu.qacc_ws[:] = g["qpos"][i], g["qvel"][i], g["qacc_ws"][i]
        last = g["last_qpos"][i].astype(np.float32)
        obs, done = emu.kitchen_step(g["action"][i], last, noise=g["noise"][i])
        assert emu.status.value == 0 and done == int(g["completed"][i])
        assert np.array_equal(last, obs[:9])
        errs.append(np.abs(obs - g["obs"][i]))
    e = np.array(errs)
    pos, vel = np.concatenate([e[:, :9], e[:, 18:39]], axis=1).max(axis=1), np.concatenate([e[:, 9:18], e[:, 39:]], axis=1).max(axis=1)
    print(f"positions p50 {np.median(pos):.2e} max {pos.max():.2e}; velocities p50 {np.median(vel):.2e} p90 {np.quantile(vel, 0.9):.2e} max {vel.max():.2e}")
    # With the portal routine in fp64 ("Mixed precision") every snapshot that is not within 1e-6 of a constraint-activation boundary is within 1e-4
    # -- the policy of tests/test_gpu_tolerance_table.py, which runs all 248 on the MI355X; here every fourth, emulated.
    gap = g["activation_gap"][::4][: len(pos)] if "activation_gap" in g.files else np.full(len(pos), np.inf)
    posed = gap >= 1e-6
    assert posed.mean() > 0.6
    assert pos[posed].max() < 1e-4 and vel[posed].max() < 1e-4, (pos[posed].max(), vel[posed].max())
    assert np.mean(pos < 1e-4) >= 0.98 and np.mean(vel < 1e-4) >= 0.98 and pos.max() < 1e-2 and vel.max() < 0.5


def test_emulated_reset_forward_matches_golden(model):
    from emu_sim import EmuSim

    from gymnasium_robotics_amd.envs.kitchen_spec import INIT_QPOS, make_kitchen_task

    g = np.load(os.path.join(GOLDEN, "kitchen_teacher.npz"))
    emu = EmuSim(model, make_kitchen_task(model, 0.01, 0.0005))
    for k in range(len(g["reset_seed"])):
        emu.qpos[:], emu.qvel[:], emu.qacc_ws[:] = INIT_QPOS, 0, 0
        last = np.zeros(9, np.float32)
        obs, _ = emu.kitchen_step(np.zeros(9, np.float32), last, noise=g["reset_noise"][k], forward_only=True)
        assert np.abs(obs - g["reset_obs"][k]).max() < 1e-6


def test_gated_engine_source_finds_the_ungated_checker_contact_set(model):
    """The kitchen scene carries 64 joint-box gates (mjcf/pair_gates.py: arm link against arm link, arm link against the world-fixed hulls).  The engine source in the lane
    emulator evaluates them; the checker knows nothing about gates.  Over random Franka configurations anywhere in the joint ranges the two must find the same geom pairs in contact."""
    from emu_sim import EmuSim

    from gymnasium_robotics_amd.envs.kitchen_spec import INIT_QPOS, make_kitchen_task
    from oracle.oracle_sim import OracleSim

    T = model.tables
    assert (np.asarray(T["devpair_gate"]).ravel() >= 0).sum() == 64 and len(np.asarray(T["gate_qadr"]).ravel()) == 3 * 64
    emu, sim = EmuSim(model, make_kitchen_task(model, 0.0, 0.0)), OracleSim(model)
    jr = np.asarray(T["jnt_range"]).reshape(-1, 2)
    rng = np.random.default_rng(4)
    with_contacts = 0
    for trial in range(24):
        q = INIT_QPOS.astype(np.float64).copy()
        q[:7] = rng.uniform(jr[:7, 0], jr[:7, 1])          # the seven arm joints anywhere in their ranges (the arm may well be inside the furniture: both sides must agree there too)
        q[7:9] = rng.uniform(0.0, 0.04, 2)
        sim.qpos[:] = q; sim.qvel[:] = 0
        sim.forward()
        want = sorted((int(c[7]), int(c[8])) for c in sim.contacts())
        emu.qpos[:] = q.astype(np.float32); emu.qvel[:] = 0; emu.qacc_ws[:] = 0
        ncon, _ = emu.physics_steps(1)
        pairs = emu.ctx("con_pair", max(ncon, 1), np.int32)[:ncon]
        got = sorted((int(T["pair_geom1"][p]), int(T["pair_geom2"][p])) for p in pairs)
        if len(want) <= 32:                                  # (the engine's contact list holds 32; beyond that the checker's list is longer by construction)
            assert got == want, (trial, got, want)
            with_contacts += len(want) > 0
    assert with_contacts >= 10
