"""The reference's own BaseRobotEnv.step (robot_env.py:114-152) with MujocoFetchEnv's _set_action / _step_callback / _get_obs and the
mujoco_utils helpers (ctrl_set_action, mocap_set_action + reset_mocap2body_xpos, robot_get_obs, get_site_xpos / xvelp / xvelr / xmat,
set_joint_qpos) EXECUTED on top of the oracle's physics (tests/ref_harness.py), against the oracle environment's restated task layer
on an identical second simulation: observations, achieved goal, reward, success flag and the post-step state must be bit-identical.
This pins SURVEY.md section 8(a) rows P1, P3-P9 of the checker against the reference code itself; what stays unpinned is the
physics (P2).  Where the reference tree is absent, the reference's side is replayed from its recording (ref_harness.Tape,
tests/golden/ref_task_layer/): the same answers, arguments checked, the host simulation's state written back after every call."""
import numpy as np
import pytest

import ref_harness


@pytest.fixture
def tape(request):
    failed = request.session.testsfailed
    t = ref_harness.Tape(request.node.name)
    yield t
    t.close(passed=request.session.testsfailed == failed)


@pytest.mark.parametrize("task,reward_type", [("FetchReach", "sparse"), ("FetchPush", "dense"), ("FetchSlide", "sparse"), ("FetchPickAndPlace", "sparse")])
def test_reference_step_on_oracle_physics_equals_the_oracle_env(fetch_models, task, reward_type, tape):
    from oracle.fetch_oracle import OracleFetchEnv

    a_env = OracleFetchEnv(fetch_models[task], task, reward_type=reward_type)      # restated task layer
    b_env = OracleFetchEnv(fetch_models[task], task, reward_type=reward_type)      # physics host for the reference's task layer
    oa, _ = a_env.reset(seed=11)
    ob, _ = b_env.reset(seed=11)
    assert np.array_equal(oa["observation"], ob["observation"])
    ref = tape.env(b_env, lambda: ref_harness.fetch_on_oracle(b_env, reward_type))
    # the reference's _get_obs on the freshly reset state
    o0 = ref._get_obs()
    assert np.array_equal(o0["observation"], oa["observation"]) and np.array_equal(o0["achieved_goal"], oa["achieved_goal"]) and np.array_equal(o0["desired_goal"], oa["desired_goal"])
    rng = np.random.default_rng(3)
    for t in range(12):
        act = rng.uniform(-1.3, 1.3, 4).astype(np.float32)                         # beyond [-1, 1]: step() clips
        if t == 5:
            act[:3] = 0
        oa, ra, ta, tra, ia = a_env.step(act)
        ob, rb, tb, trb, ib = ref.step(act)
        assert np.array_equal(ob["observation"], oa["observation"]), (t, np.abs(ob["observation"] - oa["observation"]).max())
        assert np.array_equal(ob["achieved_goal"], oa["achieved_goal"]) and np.array_equal(ob["desired_goal"], oa["desired_goal"])
        assert rb == ra and type(rb) is type(ra) and ib["is_success"] == ia["is_success"]
        assert tb is False and trb is False
        assert np.array_equal(a_env.sim.qpos, b_env.sim.qpos) and np.array_equal(a_env.sim.qvel, b_env.sim.qvel)
        assert np.array_equal(a_env.sim.ctrl, b_env.sim.ctrl) and np.array_equal(a_env.sim.mocap_pos, b_env.sim.mocap_pos) and np.array_equal(a_env.sim.mocap_quat, b_env.sim.mocap_quat)
    with pytest.raises(ValueError, match="Action dimension mismatch"):
        ref.step(np.zeros(3, np.float32))


def _same_step(a_out, b_out, a_sim, b_sim, t):
    (oa, ra, _, _, ia), (ob, rb, tb, trb, ib) = a_out, b_out
    for k in ("observation", "achieved_goal", "desired_goal"):
        assert np.array_equal(ob[k], oa[k]), (t, k, np.abs(ob[k] - oa[k]).max())
    # dense manipulation reward: -(10 d_pos + d_rot) with d_rot = 2 acos(w) of a quaternion product -- the restated product associates
    # differently and may differ in the last bit
    assert abs(float(rb) - float(ra)) <= 1e-12 and float(ib["is_success"]) == float(ia["is_success"]) and tb is False and trb is False
    assert np.array_equal(a_sim.qpos, b_sim.qpos) and np.array_equal(a_sim.qvel, b_sim.qvel) and np.array_equal(a_sim.ctrl, b_sim.ctrl)


@pytest.mark.parametrize("reward_type", ["sparse", "dense"])
def test_reference_hand_reach_step_on_oracle_physics(reward_type, tape):
    """hand_env.py:42-61 (_set_action, absolute control), reach.py:92-97,398-428 (_get_obs, reward, success) executed as is."""
    from gymnasium_robotics_amd.envs.hand import load_hand_reach_model
    from oracle.hand_oracle import OracleHandReachEnv

    model = load_hand_reach_model()
    a_env, b_env = OracleHandReachEnv(model, reward_type), OracleHandReachEnv(model, reward_type)
    a_env.reset(seed=4); b_env.reset(seed=4)
    ref = tape.env(b_env, lambda: ref_harness.hand_on_oracle(b_env, "reach", reward_type=reward_type, distance_threshold=0.01))
    o0 = ref._get_obs()
    assert np.array_equal(o0["observation"], a_env._obs()["observation"])
    rng = np.random.default_rng(1)
    for t in range(8):
        act = rng.uniform(-1.2, 1.2, 20).astype(np.float32)
        _same_step(a_env.step(act), ref.step(act), a_env.sim, b_env.sim, t)


@pytest.mark.parametrize("env_id", ["HandManipulateBlockRotateXYZ-v1", "HandManipulateBlockFullDense-v1", "HandManipulateEggRotate-v1", "HandManipulatePenRotateDense-v1"])
def test_reference_manipulate_step_on_oracle_physics(env_id, tape):
    """manipulate.py:87-142,298-316 (_goal_distance incl. the pen's ignore-z path, compute_reward, _is_success, _get_obs) executed as is."""
    from gymnasium_robotics_amd.envs.hand import load_hand_block_model
    from gymnasium_robotics_amd.envs.manipulate_spec import OBJECTS, object_of, parse_block_id
    from oracle.manipulate_oracle import OracleHandBlockEnv

    tp, tr, rt, _ = parse_block_id(env_id)
    obj = object_of(env_id)
    model = load_hand_block_model(obj=obj)
    a_env, b_env = OracleHandBlockEnv(model, tp, tr, rt, "off", obj), OracleHandBlockEnv(model, tp, tr, rt, "off", obj)
    a_env.reset(seed=2); b_env.reset(seed=2)
    ref = tape.env(b_env, lambda: ref_harness.hand_on_oracle(b_env, "manipulate", reward_type=rt, target_position=tp, target_rotation=tr, rotation_threshold=0.1,
                                                             distance_threshold=OBJECTS[obj]["distance_threshold"],
                                                             ignore_z_target_rotation=OBJECTS[obj]["ignore_z_target_rotation"]))
    assert np.array_equal(ref._get_obs()["observation"], a_env._obs()["observation"])
    rng = np.random.default_rng(5)
    for t in range(6):
        act = (0.4 * rng.uniform(-1, 1, 20)).astype(np.float32)
        _same_step(a_env.step(act), ref.step(act), a_env.sim, b_env.sim, t)


@pytest.mark.parametrize("task", ["FetchReach", "FetchPush", "FetchSlide", "FetchPickAndPlace"])
def test_reference_reset_on_oracle_physics(fetch_models, task, tape):
    """robot_env.py:154-186 (reset: seeding, _reset_sim loop, _sample_goal, _get_obs) with fetch_env.py:375-402 executed as is."""
    from oracle.fetch_oracle import OracleFetchEnv

    a_env, b_env = OracleFetchEnv(fetch_models[task], task), OracleFetchEnv(fetch_models[task], task)
    ref = tape.env(b_env, lambda: ref_harness.fetch_on_oracle(b_env))
    for seed in (0, 7, 123):
        oa, _ = a_env.reset(seed=seed)
        ob, info = ref.reset(seed=seed)
        assert info == {}
        for k in ("observation", "achieved_goal", "desired_goal"):
            assert np.array_equal(ob[k], oa[k]), (seed, k)
        assert np.array_equal(a_env.sim.qpos, b_env.sim.qpos) and np.array_equal(a_env.sim.qvel, b_env.sim.qvel)
        act = np.full(4, 0.3, np.float32)
        assert np.array_equal(ref.step(act)[0]["observation"], a_env.step(act)[0]["observation"])      # and the episode continues identically


def test_reference_hand_reach_reset_on_oracle_physics(tape):
    from gymnasium_robotics_amd.envs.hand import load_hand_reach_model
    from oracle.hand_oracle import OracleHandReachEnv

    model = load_hand_reach_model()
    a_env, b_env = OracleHandReachEnv(model), OracleHandReachEnv(model)
    ref = tape.env(b_env, lambda: ref_harness.hand_on_oracle(b_env, "reach", reward_type="sparse", distance_threshold=0.01, initial_goal=b_env.initial_goal.copy(),
                                                             palm_xpos=b_env.palm_xpos.copy()))
    for seed in (1, 22):
        oa, _ = a_env.reset(seed=seed)
        ob, _ = ref.reset(seed=seed)
        for k in ("observation", "achieved_goal", "desired_goal"):
            assert np.array_equal(ob[k], oa[k]), (seed, k)


@pytest.mark.parametrize("env_id", ["HandManipulateBlockRotateXYZ-v1", "HandManipulateBlockRotateParallel-v1", "HandManipulateEggFull-v1", "HandManipulatePenRotate-v1"])
def test_reference_manipulate_reset_on_oracle_physics(env_id, tape):
    """manipulate.py:154-224 (_reset_sim: pose randomisation, ten settle steps through _set_action + mj_step, the on-palm test) and
    :226-279 (_sample_goal from the settled pose), inside robot_env.py's reset loop, executed as is."""
    import types

    from gymnasium_robotics_amd.envs.hand import load_hand_block_model
    from gymnasium_robotics_amd.envs.manipulate_spec import OBJECTS, TARGET_POSITION_RANGE, object_of, parse_block_id
    from gymnasium_robotics_amd.envs import manipulate_spec as ms
    from oracle.manipulate_oracle import OracleHandBlockEnv

    tp, tr, rt, _ = parse_block_id(env_id)
    obj = object_of(env_id)
    model = load_hand_block_model(obj=obj)
    a_env, b_env = OracleHandBlockEnv(model, tp, tr, rt, "off", obj), OracleHandBlockEnv(model, tp, tr, rt, "off", obj)

    def build():
        ref = ref_harness.hand_on_oracle(b_env, "manipulate", reward_type=rt, target_position=tp, target_rotation=tr, rotation_threshold=0.1,
                                         distance_threshold=OBJECTS[obj]["distance_threshold"], ignore_z_target_rotation=OBJECTS[obj]["ignore_z_target_rotation"],
                                         randomize_initial_rotation=OBJECTS[obj]["randomize_initial_rotation"], randomize_initial_position=True,
                                         target_position_range=TARGET_POSITION_RANGE, parallel_quats=list(ms.canonical_parallel_quats()))
        # the object:center site sits at the origin of the free object body (manipulate_*.xml); the engine model tracks no site for these envs
        ref._model_names._site_name2id = {"object:center": 0}
        type(ref.data).site_xpos = property(lambda self: self._env.sim.qpos[self._env.qa: self._env.qa + 3].reshape(1, 3))
        return ref

    try:
        ref = tape.env(b_env, build)
        for seed in (0, 3):
            oa, _ = a_env.reset(seed=seed)
            ob, _ = ref.reset(seed=seed)
            for k in ("observation", "achieved_goal", "desired_goal"):
                assert np.allclose(ob[k], oa[k], rtol=0, atol=1e-15), (seed, k, np.abs(ob[k] - oa[k]).max())
            assert np.array_equal(a_env.sim.qpos, b_env.sim.qpos)
    finally:
        ref_harness.HandDataProxy.site_xpos = property(lambda self: self._env.sim.site_xpos.reshape(-1, 3))


@pytest.mark.parametrize("layout,reward_type,continuing,reset_target", [("UMaze", "sparse", True, False), ("Medium_Diverse_GR", "dense", False, False),
                                                                        ("Large_Diverse_G", "sparse", True, True)])
def test_reference_point_maze_on_oracle_physics(layout, reward_type, continuing, reset_target, tape):
    """point_maze.py:375-406 (reset / step), point.py:55-77 (PointEnv.step: action clip, velocity clip, do_simulation), maze_v4.py:148-242
    (Maze.make_maze), :278-418 (goal / reset sampling, noise, reward, termination, update_goal) executed as is; only gymnasium's MujocoEnv
    base class is a stand-in (see ref_harness)."""
    import os

    from gymnasium_robotics_amd.envs import maze_spec
    from gymnasium_robotics_amd.envs.point_maze import load_point_maze_model
    from oracle.maze_oracle import OraclePointMazeEnv

    base = layout.split("_")[0]
    maze = maze_spec.Maze(maze_spec.MAPS[layout], maze_spec.POINT_MAZE_SIZE_SCALING, maze_spec.POINT_MAZE_HEIGHT)
    model = load_point_maze_model(maze, base)
    a_env = OraclePointMazeEnv(model, maze, reward_type, continuing, reset_target=reset_target)
    b_env = OraclePointMazeEnv(model, maze, reward_type, continuing, reset_target=reset_target)
    xml = os.path.join(ref_harness.REF_ROOT, "gymnasium_robotics", "envs", "assets", "point", "point.xml")
    ref = tape.env(b_env, lambda: ref_harness.point_maze_on_oracle(b_env, maze_spec.MAPS[layout], reward_type, continuing, reset_target, xml))
    # the reference's own Maze against this package's
    assert np.allclose(np.array(ref.maze.unique_goal_locations), np.array(maze.unique_goal_locations)) and np.allclose(np.array(ref.maze.unique_reset_locations), np.array(maze.unique_reset_locations))
    rng = np.random.default_rng(0)
    events = {"success": 0, "terminated": 0, "goal_redrawn": 0}
    for seed in (0, 9):
        oa, ia = a_env.reset(seed=seed, options={"goal_cell": np.array([1, 1]), "reset_cell": np.array([1, 2])} if seed == 9 and layout == "UMaze" else None)
        ob, ib = ref.reset(seed=seed, options={"goal_cell": np.array([1, 1]), "reset_cell": np.array([1, 2])} if seed == 9 and layout == "UMaze" else None)
        for k in ("observation", "achieved_goal", "desired_goal"):
            assert np.array_equal(ob[k], oa[k]), (seed, k)
        assert ib["success"] == ia["success"]
        for t in range(150):
            act = rng.uniform(-1.5, 1.5, 2).astype(np.float32)
            if t >= 10:                           # then steer at the goal (straight-line: works where no wall is in between) so that success / termination / goal redraw happen
                act = np.clip(6 * (a_env.goal - a_env.sim.qpos[:2]) - 1.5 * a_env.sim.qvel[:2], -1, 1).astype(np.float32)
            g_before = a_env.goal.copy()
            sa, sb = a_env.step(act), ref.step(act)
            for k in ("observation", "achieved_goal", "desired_goal"):
                assert np.array_equal(sb[0][k], sa[0][k]), (seed, t, k)
            assert abs(float(sb[1]) - float(sa[1])) <= 1e-15 and bool(sb[2]) == bool(sa[2]) and bool(sb[3]) == bool(sa[3]) and sb[4]["success"] == sa[4]["success"]   # dense: exp(-d), last bit of libm vs numpy
            assert np.array_equal(ref.goal, a_env.goal)
            events["success"] += bool(sa[4]["success"]); events["terminated"] += bool(sa[2]); events["goal_redrawn"] += not np.array_equal(g_before, a_env.goal)
            if sa[2]:
                break
    if layout == "UMaze":
        assert events["success"] > 0, events                # neighbouring cells: the goal is reached


@pytest.mark.parametrize("layout,reward_type,continuing,reset_target", [("UMaze", "sparse", True, False), ("Large_Diverse_GR", "sparse", True, False),
                                                                        ("Medium_Diverse_G", "dense", False, False), ("Large_Diverse_G", "sparse", True, True)])
def test_reference_ant_maze_on_oracle_physics(layout, reward_type, continuing, reset_target, tape):
    """ant_maze_v5.py:282-320 (AntMazeEnv.reset / step / _get_obs / update_target_site_pos) and everything they inherit from MazeEnv
    (maze_v4.py:148-242 Maze.make_maze at scaling 4 / height 0.5, :278-418 goal / reset sampling, noise, reward, termination, update_goal) executed
    as is on the oracle's physics; gymnasium's AntEnv [3P] is the documented-behaviour stand-in of ref_harness (obs = qpos | qvel, frame_skip 5,
    reset_noise_scale 0).  Includes BASELINE.json configs[3]'s own layout (Large_Diverse_GR)."""
    import os

    from gymnasium_robotics_amd.envs import maze_spec
    from gymnasium_robotics_amd.envs.point_maze import load_point_maze_model
    from oracle.maze_oracle import OracleAntMazeEnv

    base = layout.split("_")[0]
    maze = maze_spec.Maze(maze_spec.MAPS[layout], maze_spec.ANT_MAZE_SIZE_SCALING, maze_spec.ANT_MAZE_HEIGHT)
    model = load_point_maze_model(maze, base, None, "ant")
    a_env = OracleAntMazeEnv(model, maze, reward_type, continuing, reset_target=reset_target)
    b_env = OracleAntMazeEnv(model, maze, reward_type, continuing, reset_target=reset_target)
    xml = os.path.join(ref_harness.REF_ROOT, "gymnasium_robotics", "envs", "assets", "point", "point.xml")   # make_maze only needs a worldbody to append the wall geoms to
    ref = tape.env(b_env, lambda: ref_harness.ant_maze_on_oracle(b_env, maze_spec.MAPS[layout], reward_type, continuing, reset_target, xml))
    assert np.allclose(np.array(ref.maze.unique_goal_locations), np.array(maze.unique_goal_locations)) and np.allclose(np.array(ref.maze.unique_reset_locations), np.array(maze.unique_reset_locations))
    assert ref.maze.maze_size_scaling == 4 and ref.maze.maze_height == 0.5
    rng = np.random.default_rng(0)
    events = {"success": 0, "terminated": 0, "goal_redrawn": 0}
    for seed in (0, 9):
        opts = {"goal_cell": np.array([1, 1]), "reset_cell": np.array([1, 2])} if seed == 9 and layout == "UMaze" else None
        oa, ia = a_env.reset(seed=seed, options=opts)
        ob, ib = ref.reset(seed=seed, options=opts)
        assert ob["observation"].shape == (27,) and ob["achieved_goal"].shape == (2,)
        for k in ("observation", "achieved_goal", "desired_goal"):
            assert np.array_equal(ob[k], oa[k]), (seed, k)
        assert ib["success"] == ia["success"]
        assert np.array_equal(ref.ant_env.model.site_pos[0], np.append(a_env.goal, 1.0))      # update_target_site_pos: z = height / 2 * scaling
        for t in range(40):
            act = rng.uniform(-1, 1, 8).astype(np.float32)
            if t == 20:      # carry both ants to their goal (same state edit on both simulations) so that success / termination / goal redraw happen
                for e in (a_env, b_env):
                    e.sim.qpos[:2] = a_env.goal + 0.1
                    e.sim.forward()
            g_before = a_env.goal.copy()
            sa, sb = a_env.step(act), ref.step(act)
            for k in ("observation", "achieved_goal", "desired_goal"):
                assert np.array_equal(sb[0][k], sa[0][k]), (seed, t, k)
            assert abs(float(sb[1]) - float(sa[1])) <= 1e-15 and bool(sb[2]) == bool(sa[2]) and bool(sb[3]) == bool(sa[3]) and sb[4]["success"] == sa[4]["success"]
            assert np.array_equal(ref.goal, a_env.goal)
            events["success"] += bool(sa[4]["success"]); events["terminated"] += bool(sa[2]); events["goal_redrawn"] += not np.array_equal(g_before, a_env.goal)
            if sa[2]:
                break
    assert events["success"] > 0, events
    assert (events["terminated"] > 0) == (not continuing) and (events["goal_redrawn"] > 0) == (continuing and reset_target), events


# manipulate_touch_sensors.py:113-138 (_get_obs with the 92 touch readings raw / > 0 / log(x + 1)) executed as is on the oracle's sensor
# values; the step itself is the reference's BaseRobotEnv.step.
def _touch_case(mode, tape):
    from gymnasium_robotics_amd.envs.hand import load_hand_block_model
    from oracle.manipulate_oracle import OracleHandBlockEnv

    model = load_hand_block_model(touch=True)
    a_env, b_env = OracleHandBlockEnv(model, "ignore", "xyz", "sparse", mode, "block"), OracleHandBlockEnv(model, "ignore", "xyz", "sparse", mode, "block")
    a_env.reset(seed=6); b_env.reset(seed=6)

    def build():
        ref = ref_harness.hand_on_oracle(b_env, "manipulate", reward_type="sparse", target_position="ignore", target_rotation="xyz", rotation_threshold=0.1,
                                         distance_threshold=0.01, ignore_z_target_rotation=False, touch_get_obs=mode, _touch_sensor_id=list(range(92)))
        from gymnasium_robotics.envs.shadow_dexterous_hand import manipulate_touch_sensors as mts

        ref.__class__ = mts.MujocoManipulateTouchSensorsEnv
        type(ref.data).sensordata = property(lambda self: self._env.sim.touch)
        return ref
    return a_env, b_env, tape.env(b_env, build)


@pytest.mark.parametrize("mode", ["sensordata", "boolean", "log"])
def test_reference_touch_observation(mode, tape):
    ref_harness.install()
    a_env, b_env, ref = _touch_case(mode, tape)
    rng = np.random.default_rng(2)
    fired = 0
    for t in range(5):
        act = (0.3 * rng.uniform(-1, 1, 20)).astype(np.float32)
        sa, sb = a_env.step(act), ref.step(act)
        assert sb[0]["observation"].shape == (153,) and np.array_equal(sb[0]["observation"], sa[0]["observation"]), (t, np.abs(sb[0]["observation"] - sa[0]["observation"]).max())
        assert np.array_equal(sb[0]["achieved_goal"], sa[0]["achieved_goal"]) and float(sb[1]) == float(sa[1])
        fired += int((sa[0]["observation"][61:] > 0).sum())
    assert fired > 0


@pytest.mark.parametrize("reward_type", ["dense", "sparse"])
def test_reference_adroit_hammer_on_oracle_physics(reward_type, tape):
    """adroit_hammer.py:291-378 executed as is (action scaling, do_simulation(a, 5), the 46-vector observation with quat2euler and the clipped
    velocities / touch reading, dense and sparse reward, success flag, reset_model's board-height draw written to model.body_pos) on the oracle
    physics: identical to the restated task layer (oracle/adroit_oracle.py) step for step."""
    from gymnasium_robotics_amd.envs.adroit_spec import load_adroit_hammer_model
    from oracle.adroit_oracle import OracleAdroitHammerEnv

    ref_harness.install()
    model = load_adroit_hammer_model()
    a_env, b_env = OracleAdroitHammerEnv(model, reward_type), OracleAdroitHammerEnv(model, reward_type)
    ref = tape.env(b_env, lambda: ref_harness.adroit_hammer_on_oracle(b_env, reward_type))
    rng = np.random.default_rng(4)
    for seed in (0, 5):
        oa, _ = a_env.reset(seed=seed)
        ob, _ = ref.reset(seed=seed)
        assert ob.shape == (46,) and np.array_equal(ob, oa)
        assert a_env.board_z == b_env.board_z and 0.1 <= a_env.board_z <= 0.25
        for t in range(40):
            act = rng.uniform(-1.2, 1.2, 26).astype(np.float32)
            sa, sb = a_env.step(act), ref.step(act)
            assert np.array_equal(sb[0], sa[0]), (seed, t, np.abs(sb[0] - sa[0]).max())
            assert float(sb[1]) == float(sa[1]) and bool(sb[4]["success"]) == bool(sa[4]["success"]) and sb[2] is False and sb[3] is False


@pytest.mark.parametrize("task", ["door", "pen", "relocate"])
@pytest.mark.parametrize("reward_type", ["dense", "sparse"])
def test_reference_adroit_door_pen_relocate_on_oracle_physics(task, reward_type, tape):
    """adroit_door.py:281-392, adroit_pen.py:288-419, adroit_relocate.py:290-410 executed as they are (action scaling, do_simulation(a, 5), the 39 /
    45 / 39-vector observations, dense and sparse rewards, success flags, reset_model's draws written to model.body_pos / body_quat / site_pos,
    get_env_state / set_env_state) on the oracle physics: identical to the restated task layer (oracle/adroit_oracle.py) step for step, bit for bit."""
    from gymnasium_robotics_amd.envs.adroit_spec import load_adroit_model
    from oracle.adroit_oracle import OracleAdroitEnv

    ref_harness.install()
    model = load_adroit_model(task)
    a_env, b_env = OracleAdroitEnv(model, reward_type, task), OracleAdroitEnv(model, reward_type, task)
    ref = tape.env(b_env, lambda: ref_harness.adroit_on_oracle(b_env, task, reward_type))
    rng = np.random.default_rng(4)
    nu = model.dim("nu")
    for seed in (0, 5):
        oa, _ = a_env.reset(seed=seed)
        ob, _ = ref.reset(seed=seed)
        assert ob.shape == oa.shape == ({"door": 39, "pen": 45, "relocate": 39}[task],) and np.array_equal(ob, oa)
        assert np.array_equal(a_env.model_edit, b_env.model_edit) and np.array_equal(a_env.target_pos, b_env.target_pos)
        for t in range(25):
            act = rng.uniform(-1.2, 1.2, nu).astype(np.float32)
            sa, sb = a_env.step(act), ref.step(act)
            assert np.array_equal(sb[0], sa[0]), (seed, t, np.abs(sb[0] - sa[0]).max())
            assert float(sb[1]) == float(sa[1]) and bool(sb[4]["success"]) == bool(sa[4]["success"]) and sb[2] is False and sb[3] is False
    # the reference's get_env_state -> set_env_state round trip lands on the same state and model edit (set_state runs mj_forward, so the site /
    # body poses in the observation move from the pre-integration to the post-integration configuration: the joint part is unchanged)
    st = ref.get_env_state()
    before, edit = ref._get_obs(), b_env.model_edit.copy()
    ref.set_env_state({k: st[k] for k in ref._state_space.spaces})
    st2 = ref.get_env_state()
    assert all(np.allclose(st2[k], st[k], atol=1e-12) for k in ref._state_space.spaces) and np.allclose(b_env.model_edit, edit, atol=1e-12)
    nj = {"door": 27, "pen": 24, "relocate": 30}[task]
    assert np.array_equal(ref._get_obs()[:nj], before[:nj])


def test_reference_relocate_reset_keeps_the_components_it_does_not_redraw(tape):
    """adroit_relocate.py:353-356: reset_model redraws model.body_pos[Object] x / y only; a z that set_env_state wrote (:405-407) persists across resets in the
    reference.  The restated task layer (adroit_spec.sample_reset_batch(current=...), used by the oracle env and by AdroitVecEnv) must do the same."""
    from gymnasium_robotics_amd.envs.adroit_spec import load_adroit_model
    from oracle.adroit_oracle import OracleAdroitEnv

    ref_harness.install()
    model = load_adroit_model("relocate")
    a_env, b_env = OracleAdroitEnv(model, "dense", "relocate"), OracleAdroitEnv(model, "dense", "relocate")
    ref = tape.env(b_env, lambda: ref_harness.adroit_on_oracle(b_env, "relocate", "dense"))
    a_env.reset(seed=3); ref.reset(seed=3)
    st = ref.get_env_state()
    st["obj_pos"] = st["obj_pos"] + np.array([0.0, 0.0, 0.07])         # the ball 7 cm higher: lands in model.body_pos[Object, 2]
    ref.set_env_state({k: st[k] for k in ref._state_space.spaces})
    z_ref = b_env.model_edit[2]
    a_env.set_model_edit(b_env.model_edit.copy(), b_env.target_pos.copy())     # the same edit on the restated env
    oa, _ = a_env.reset(seed=8)
    ob, _ = ref.reset(seed=8)
    assert b_env.model_edit[2] == z_ref and abs(z_ref - model.info["shift_pos0"][2]) > 0.05        # the reference kept its z ...
    assert np.array_equal(a_env.model_edit, b_env.model_edit) and np.array_equal(oa, ob)           # ... and so does the restatement (x / y redrawn identically)


@pytest.mark.parametrize("kwargs", [{}, {"tasks_to_complete": ["microwave", "kettle"], "remove_task_when_completed": False}])
def test_reference_kitchen_on_oracle_physics(kwargs, tape):
    """franka_env.py:92-171 and kitchen_env.py:340-437 executed as they are (velocity command on the previous noisy reading, position / velocity
    bounds read from franka_config.xml by the reference's own parser, do_simulation(ctrl, 40), both _get_obs with their PCG64 noise draws,
    compute_reward, task bookkeeping, termination) on the oracle physics: identical to the restated task layer (oracle/kitchen_oracle.py), bit for bit."""
    from gymnasium_robotics_amd.envs.kitchen_spec import load_kitchen_model
    from oracle.kitchen_oracle import OracleKitchenEnv

    ref_harness.install()
    model = load_kitchen_model()
    a_env, b_env = OracleKitchenEnv(model, **kwargs), OracleKitchenEnv(model, **kwargs)
    ref = tape.env(b_env, lambda: ref_harness.kitchen_on_oracle(b_env))
    rng = np.random.default_rng(1)
    for seed in (0, 3):
        (oa, ia), (ob, ib) = a_env.reset(seed=seed), ref.reset(seed=seed)
        assert ob["observation"].shape == (59,) and np.array_equal(oa["observation"], ob["observation"]) and sorted(ia["tasks_to_complete"]) == sorted(ib["tasks_to_complete"])
        for t in range(10):
            act = rng.uniform(-1.3, 1.3, 9)
            if t == 4:   # put the microwave door at its goal: a completion (and, with the two-task list, not yet termination) on both sides
                a_env.sim.qpos[22] = b_env.sim.qpos[22] = -0.75
            sa, sb = a_env.step(act), ref.step(act)
            assert np.array_equal(sa[0]["observation"], sb[0]["observation"]), (seed, t, np.abs(sa[0]["observation"] - sb[0]["observation"]).max())
            assert sa[1] == sb[1] and sa[2] == sb[2] and sb[3] is False and sorted(sa[4]["tasks_to_complete"]) == sorted(sb[4]["tasks_to_complete"])
            assert sa[4]["step_task_completions"] == sb[4]["step_task_completions"] and sa[4]["episode_task_completions"] == sb[4]["episode_task_completions"]
            for k in sa[0]["achieved_goal"]:
                assert np.array_equal(sa[0]["achieved_goal"][k], sb[0]["achieved_goal"][k]) and np.array_equal(sa[0]["desired_goal"][k], sb[0]["desired_goal"][k])
        assert "microwave" in sa[4]["episode_task_completions"]
