"""Cameras without a device: the compiler's bookkeeping rows for tests/camera_cases.py XML, BatchedSim's camera names and the argument errors render() raises before it
touches the GPU."""
import numpy as np
import pytest

import camera_cases as K
import engine_matrix_cases as C
from gymnasium_robotics_amd.mjcf import mathutil as mu


@pytest.fixture(scope="module")
def model():
    return C.compile_xml(K.XML)


def test_compiler_rows_fused_pose_default_class_and_document_order(model):
    assert model.names["camera"] == {"eye": 0, "overview": 1, "_camera2": 2}
    eye, overview, chase = model.info["camera"]
    assert "mount" not in model.names["body"] and eye["body"] == model.names["body"]["arm"] and overview["body"] == chase["body"] == 0
    turn = mu.euler2quat(np.array([0.0, 0.0, np.pi / 2]), "xyz")      # mount in arm: pos (0.5, 0, 0.1), a quarter turn about z
    assert np.allclose(eye["pos"], [0.5, 0.02, 0.1], atol=1e-12)
    assert np.allclose(eye["quat"], mu.quat_normalize(mu.quat_mul(turn, mu.xyaxes2quat(np.array([-1.0, 0, 0, 0, -1, 0.4])))), atol=1e-12)
    assert (eye["fovy"], overview["fovy"], chase["fovy"]) == (45.0, 55.0, 45.0)
    assert (eye["mode"], chase["mode"], chase["target"], eye["resolution"]) == ("fixed", "targetbody", "arm", None)
    assert np.allclose(overview["pos"], [0.5, 0.2, 2.0])


def test_camera_names_and_argument_errors(model):
    import gymnasium_robotics_amd as grx

    sim = grx.BatchedSim(model, 4, outputs=("xpos", "xquat"))
    assert sim.camera_id("overview") == 1
    assert list(sim.cameras_unserved) == ["_camera2"] and "targetbody" in sim.cameras_unserved["_camera2"]
    with pytest.raises(KeyError, match="no camera named 'nose'"):
        sim.render("nose", 8, 8)
    with pytest.raises(ValueError, match="fixed cameras only"):
        sim.render(["eye", "_camera2"], 8, 8)
    for h, w in ((0, 8), (8, 1025)):
        with pytest.raises(ValueError, match="outside 1 .. 1024"):
            sim.render("eye", h, w)
    with pytest.raises(ValueError, match="1 .. 16 cameras"):
        sim.render(["eye"] * 17, 8, 8)
    with pytest.raises(ValueError, match="exclude_body must be one body or name 2"):
        sim.render(["eye", "overview"], 8, 8, exclude_body=[1, 1, 1])
    with pytest.raises(ValueError, match=r"needs the output\(s\) \['xquat'\]"):
        grx.BatchedSim(model, 4, outputs=("xpos",)).render("eye", 8, 8)
