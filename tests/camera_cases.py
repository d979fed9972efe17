"""What tests/test_cpu_camera.py and tests/test_gpu_camera.py share: the small MJCF with its three cameras, the pixel fan in fp64 from the definition (module docstring of
gymnasium_robotics_amd/sim.py, CAMERAS) and the look-at frame.  The reference and the acceptance rule are those of tests/ray_cases.py."""
import numpy as np

from gymnasium_robotics_amd.mjcf import mathutil as mu

# `eye` rides on a static child of the hinged body `arm`: the compiler fuses `mount` into `arm`.  `overview` takes its fovy from a default class.  The third camera has no name
# and a mode render() does not serve.
XML = """<mujoco><default><default class="wide"><camera fovy="55"/></default></default><worldbody>
  <geom name="floor" type="plane" size="3 3 0.1"/>
  <geom name="post" type="box" size="0.1 0.15 0.5" pos="1.3 0.2 0.5"/>
  <geom name="ball" type="sphere" size="0.2" pos="0.4 1.2 0.6"/>
  <body name="arm" pos="0 0 1"><joint name="swing" type="hinge" axis="0 0 1"/><geom name="link" type="capsule" size="0.05 0.2" pos="0.25 0 0" euler="0 90 0" mass="1"/>
    <body name="mount" pos="0.5 0 0.1" euler="0 0 90"><geom name="head" type="sphere" size="0.06" mass="0.1"/>
      <camera name="eye" pos="0.02 0 0" xyaxes="-1 0 0 0 -1 0.4"/></body></body>
  <camera name="overview" class="wide" pos="0.5 0.2 2" xyaxes="1 0 0 0 1 0.15"/>
  <camera mode="targetbody" target="arm" pos="1 1 1"/>
</worldbody></mujoco>"""


def fan(pos, xmat, fovy, height, width):
    """(o, d) [H * W, 3] in fp64: the centre ray of every pixel, row-major from the top row, of a camera at pos with the frame xmat (camera -> world; it looks along -z)"""
    t = np.tan(np.radians(fovy) / 2.0)
    r, c = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    local = np.stack([(2.0 * (c + 0.5) / width - 1.0) * t * width / height, (1.0 - 2.0 * (r + 0.5) / height) * t, -np.ones(r.shape)], axis=-1).reshape(-1, 3)
    return np.broadcast_to(np.asarray(pos, dtype=np.float64), local.shape).copy(), local @ np.asarray(xmat, dtype=np.float64).reshape(3, 3).T


def look_at(eye, target):
    """the frame [9] of a camera at eye that looks at target, its +y as close to the world's +z as that allows"""
    back = np.asarray(eye, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    back /= np.linalg.norm(back)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(back, right), back], axis=1).reshape(9)


def pose(row, xpos, xquat):
    """the world pose (pos [3], xmat [9]) of the camera of the compiler's row, composed in fp64 from its body's pose in xpos / xquat [nbody, 3 / 4]"""
    B = mu.quat2mat(xquat.reshape(-1, 4)[row["body"]])
    return xpos.reshape(-1, 3)[row["body"]] + B @ row["pos"], (B @ mu.quat2mat(np.asarray(row["quat"]))).reshape(9)

