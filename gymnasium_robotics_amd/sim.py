"""BatchedSim: the physics alone -- ``mujoco.mj_step`` / ``mujoco.mj_forward`` for N worlds of a caller's own MJCF model on the device, with no task baked in.

The reference's ``MujocoRobotEnv`` / ``MujocoFetchEnv`` (gymnasium_robotics/envs/robot_env.py:280-345) exist to be subclassed with one's own XML: the
subclass writes ``data.ctrl`` / ``data.mocap_pos``, calls ``mj_step(model, data, nstep=n_substeps)`` (robot_env.py:341) and reads ``data.qpos``, ``data.site_xpos`` and
``mujoco_utils.get_site_xvelp``.  This class is that loop for a batch: the state rows are device tensors the caller writes in place, ``step`` / ``forward`` enqueue one launch
of the generic engine kernel (grx_sim_step, include/grx_capi.h) on torch's current stream, and the requested ``MjData`` fields are device tensors afterwards.

    sim = grx.BatchedSim("my_robot.xml", num_worlds=4096, outputs=("site_xpos", "site_xvelp"))
    sim.reset()
    sim.ctrl[:] = policy(obs)                 # any torch op on the current stream
    sim.step(nstep=20)
    tip = sim.site_xpos[:, sim.site_id("tip")]

Outputs are what ``MjData`` holds at that moment: after ``step`` the derived fields belong to the position / velocity stage of the LAST substep, before its integration (the
one-substep-stale kinematics the reference's environments read after ``mj_step``), ``qpos`` / ``qvel`` are the integrated state; after ``forward`` they belong to the state as
given.  ``site_xvelp`` / ``site_xvelr`` are the site Jacobian of that pass times the current ``qvel`` (``get_site_xvelp`` / ``get_site_xvelr``).
``sensordata`` (the raw ``mjSENS_TOUCH`` readings) belongs to that same pass: it is made from the contact list and row forces the contact outputs report.  Under RK4 that is the
forward pass of the FOURTH stage of the last substep, at the stage's trial state, not the first stage's at the substep's start; this has not been compared with MuJoCo's own
``sensordata`` under RK4.

The dynamics of the same pass are outputs too: ``qM`` (dense ``mj_fullM``), ``qfrc_bias`` / ``qfrc_passive`` / ``qfrc_actuator`` / ``qfrc_smooth`` / ``qfrc_constraint``,
``qacc_smooth`` / ``qacc``, and ``site_jacp`` / ``site_jacr``: ``mj_jacSite`` of the sites named in ``jac_sites`` (at most 16; ``sim.jac_row(name)`` is a site's row), shape
[N, len(jac_sites), 3, nv].  Requesting one of them routes the launch through grx_sim_step_dyn; a simulation that requests none calls grx_sim_step as before.

    sim = grx.BatchedSim("my_robot.xml", 4096, outputs=("qfrc_bias", "site_jacp"), jac_sites=("tip",))
    J = sim.site_jacp[:, sim.jac_row("tip")]                       # [N, 3, nv]

The CONTACT LIST of the same pass: ``contacts`` names any of ``sim.CONTACTS`` -- ``contact_geom`` [N, C, 2] (``contact.geom1`` / ``geom2``, geom ids of the compiled model:
``sim.geom_id(name)``), ``contact_dim`` [N, C], ``contact_efc_address`` [N, C] (-1: no constraint rows), ``contact_dist`` [N, C], ``contact_pos`` [N, C, 3], ``contact_frame``
[N, C, 9] (the normal, then the two tangents) and ``contact_force`` [N, C, 6] (``mj_contactForce``: normal, two tangential, torsional, two rolling, in the contact frame).
C = ``sim.contact_capacity``.  World w holds ``ncon[w]`` contacts in its first slots, in the ENGINE's order (sorted by candidate pair; not MuJoCo's order: match by geom pair and
position); the remaining slots are filled (geom -1, dim 0, efc_address -1, floats 0).  Requesting one routes the launch through grx_sim_step_con.

    sim = grx.BatchedSim("my_robot.xml", 4096, outputs=("ncon",), contacts=("contact_geom", "contact_frame", "contact_force"))
    sim.step(nstep=20)
    down = (sim.contact_geom == sim.geom_id("foot")).any(-1)                                   # [N, C]: the slots that involve the foot
    frame = sim.contact_frame.view(4096, -1, 3, 3)                                             # rows: normal, tangent 1, tangent 2, in world coordinates
    f_world = (frame.transpose(-1, -2) @ sim.contact_force[..., :3, None]).squeeze(-1)         # [N, C, 3]: frame' force[:3], the force on the pair's second geom

``xpos`` / ``xquat`` index the COMPILED model's bodies: the compiler merges static children into their parents, ``sim.model.names["body"]`` maps the surviving names to rows.
Sites keep their identity whatever body they end up on: they are the stable handle for "where is this point of my robot".

PER-WORLD MODEL PARAMETERS (domain randomization): ``model_params`` names the model tables whose values differ from world to world, any of ``sim.PARAMS``.  Each is a device
tensor ``sim.params.<name>`` of shape [N, ...], initialised to the model's own fp32 values; write it with any torch op, then ``sim.commit_params()`` makes the values take effect
for the launches that follow.  The meaning is that of writing the same ``MjModel`` fields in place, world by world, WITHOUT ``mj_setConst``: what the compiler derived from them
(``dof_invweight0``, ``geom_invweight0``, ``eq_invweight``, ``tendon_invweight0``, ``meaninertia``, the structural counts) keeps the nominal model's value -- exactly what the fp64 oracle
does when the same table is written through ``OracleSim.model_table``, which is the operational definition.  The structure stays the nominal model's: a world whose row breaks a rule
(a non-finite value, ``dof_frictionloss`` switched on or off, a negative mass, ... include/grx_capi.h) keeps the parameters of its last good commit and ``sim.params_invalid[w]`` says
which rule; a commit never raises and never synchronises.  Friction is a property of the candidate PAIR in the compiled model: ``sim.pair_ids("geom")`` gives the rows.

    sim = grx.BatchedSim("my_robot.xml", 4096, model_params=("body_mass", "dof_damping", "pair_friction", "gravity"))
    sim.params.body_mass *= torch.empty_like(sim.params.body_mass).uniform_(0.5, 2.0)
    sim.params.pair_friction[:, sim.pair_ids("foot"), 0] = torch.empty(4096, 1, device="cuda").uniform_(0.5, 1.5)
    sim.params.gravity[:, 2] = -9.81 * torch.empty(4096, device="cuda").uniform_(0.9, 1.1)
    sim.commit_params()
    assert not sim.params_invalid.any()

APPLIED FORCES, the one input that is not an actuator: ``applied`` names any of ``sim.APPLIED``.  ``qfrc_applied`` [N, nv] and ``xfrc_applied`` [N, nbody, 6] are fp32 tensors the
caller writes in place (zero-initialised, held over the substeps of a launch as ``ctrl`` is, never written by a launch, zeroed by ``reset``), with MuJoCo's meaning: in every
forward pass ``qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator + qfrc_applied + sum_b jacp_b' f_b + jacr_b' t_b``, where ``xfrc_applied[b] = (f_b, t_b)`` is a force and a
torque in world coordinates (force first) at ``xipos[b]``, the centre of mass of COMPILED body b (rows as ``xpos``; row 0, the world, is ignored).  ``xipos`` [N, nbody, 3] is
``data.xipos`` of the same pass as ``xpos``: a force at a point p is ``(f, (p - xipos) x f)``.  ``qfrc_bias`` / ``qfrc_passive`` / ``qfrc_actuator`` do not contain the applied
terms.  Naming one routes the launch through grx_sim_step_frc.  Non-finite applied values are the caller's error and behave as a non-finite ``ctrl`` does.

    sim = grx.BatchedSim("my_robot.xml", 4096, applied=("xfrc_applied", "xipos"))
    sim.xfrc_applied[:, sim.body_id("torso"), :3] = 50.0 * torch.randn(4096, 3, device="cuda")     # a shove through the torso's centre of mass
    sim.step(nstep=20)

SENSORS (``MjData.sensordata`` for the MJCF's ``<sensor>`` children): ``sensors`` names sensors of the MJCF, or is ``"all"`` -- every sensor of a served type, in MJCF order, with
``sim.sensors_unserved`` a dict name -> reason for the rest.  ``sim.sensor_data`` is [N, ndata] float32, ``sim.sensor(name)`` the [N, dim] view of one sensor, ``sim.sensor_adr(name)``
its ``(adr, dim)``.  Served: ``jointpos`` / ``jointvel`` (hinge and slide joints), ``actuatorpos`` / ``actuatorvel`` (gear times the joint's), ``actuatorfrc`` (the actuator's scalar
force before the gear), ``jointactuatorfrc``, and on a site or an ``xbody`` of the compiled model ``framepos``, ``framequat``, ``framexaxis`` / ``yaxis`` / ``zaxis``, ``framelinvel``,
``frameangvel``, ``framelinacc``, ``frameangacc``; on a site ``velocimeter``, ``gyro``, ``accelerometer``.  With p, R the object's position and rotation and Jp, Jr the Jacobians of
the material point p: u = Jp qvel, omega = Jr qvel, c = Jp qacc + (d/dt Jp) qvel, alpha = Jr qacc + (d/dt Jr) qvel; velocimeter = R'u, gyro = R'omega, framelinacc = c - g,
accelerometer = R'(c - g), frameangacc = alpha; on a site ``force`` / ``torque`` (BODY WRENCHES below).  ``- g`` is MuJoCo's convention that the world body accelerates with ``-gravity`` (an accelerometer at rest reads +9.81 along world
z); it is the DEFINITION of ``framelinacc`` here as well.  A world that names ``gravity`` among ``model_params`` reads its own committed row.  A positive ``cutoff`` clamps a reading to
[-cutoff, cutoff] (not the quaternion and axis types); ``noise`` is ignored.  Refused by name, with the reason: ``touch`` (``outputs=("sensordata",)`` with ``touch_filter``),
``rangefinder`` (``sim.rangefinder()``), ``force`` / ``torque`` on anything but a site or without ``cfrc_int`` among ``body_dynamics``, frame sensors on a ``body`` (the inertial frame),
``geom`` or ``camera``, any ``reftype``, every other type, and an ``xbody`` the compiler merged into its parent or a site ``keep_sites`` dropped.
WHICH PASS: all readings belong to ONE forward pass, with that pass's own qvel and qacc.  After ``forward()``: that pass.  After ``step(n)`` of an Euler model: the last substep's pass,
before its integration.  Of an RK4 model: the FIRST stage's pass of the last substep -- ``mj_step`` runs ``mj_forward`` with sensors, then ``mj_RungeKutta`` with the sensors skipped --
which differs on purpose from the fourth-stage pass of the other outputs.  Either way the readings after ``step(n)`` are those of ``forward()`` at the state ``step(n - 1)`` left.
Sensors are not state: ``reset()``'s ``forward()`` refreshes them, ``get_state`` / ``set_state`` do not carry them.  Naming one routes the launch through grx_sim_step_sns.

    sim = grx.BatchedSim("quadruped.xml", 4096, sensors=("imu_acc", "imu_gyro", "imu_quat", "hip_pos", "hip_vel"))
    sim.step(nstep=5)
    obs = torch.cat([sim.sensor_data, sim.ctrl], dim=1)                                            # or sim.sensor("imu_acc"): [N, 3]

BODY WRENCHES (what ``mj_rnePostConstraint`` forms): ``body_dynamics`` names any of ``sim.BODY_DYNAMICS``; rows are the compiled model's bodies, as for ``xpos``, fp32, every
element written by each launch.  ``subtree_com`` [N, nbody, 3] is ``data.subtree_com`` of the same pass as ``xpos`` (from ``xipos`` and the world's own committed ``body_mass``).  The
other three are [N, nbody, 6] spatial vectors in MuJoCo's layout -- rotation part first (torque then force, angular then linear), world orientation, about
``subtree_com[root(b)]`` with root = ``body_rootid``.  ``cfrc_ext[b]`` sums ``xfrc_applied[b]`` acting at ``xipos[b]`` and every contact of the pass that has constraint rows, with the sign
of ``mj_contactForce``: + on the body of the pair's second geom, - on the first, each about its own root's centre of mass; the torque is ``(contact_pos - com) x f`` plus the
torsional term along the normal (condim >= 4) and the rolling terms along the tangents (condim 6); row 0 (the world) receives the reactions of world-geom contacts.
``cacc[b]`` is the spatial acceleration: ``cacc[0] = (0, -gravity)``, ``cacc[b] = cacc[parent] + sum cdof_dot qvel + sum cdof qacc`` over b's own dofs.  ``cfrc_int[b]`` = sum over
e in subtree(b) of ``cinert_e cacc_e + cvel_e x* (cinert_e cvel_e) - cfrc_ext_e``: the wrench b's parent exerts on b through their joint.  DEVIATION: the forces of weld, connect and
joint EQUALITY constraints are not added to ``cfrc_ext`` (recent MuJoCo releases add connect / weld forces there); the definition above is self-contained.  WHICH PASS: that of
``qfrc_bias`` and the contact outputs -- the last forward pass, under RK4 the fourth stage's; after ``step(n)`` the rows are those of ``forward()`` at the state ``step(n - 1)`` left.  Not
state: ``reset()`` refreshes them, ``get_state`` / ``set_state`` ignore them.  The ``force`` and ``torque`` SENSORS (on a site, dim 3, cutoff clamps) read them: with b the site's body,
``(tau, f) = cfrc_int[b]``, p / R the site's position / rotation and c = ``subtree_com[root(b)]``, force = ``R' f`` and torque = ``R' (tau - (p - c) x f)``.  They follow the sensor
block's pass rule (Euler: the last pass; RK4: the FIRST stage of the last substep, so under RK4 they differ from the ``cfrc_int`` output by design).  They are
served in a simulation whose ``body_dynamics`` names ``cfrc_int``; in any other they stay refused by name, with that reason (``sensors="all"`` lists them in ``sensors_unserved``), so a
simulation that asks for no body output runs the kernels and gets the sensor columns it had.  Naming a body output routes the launch through grx_sim_step_wrn.

    sim = grx.BatchedSim("humanoid.xml", 4096, body_dynamics=("cfrc_ext", "cfrc_int", "subtree_com"), sensors=("left_foot_force",))
    sim.step(nstep=5)
    contact_cost = 5e-7 * sim.cfrc_ext.clamp(-1, 1).square().sum((1, 2))

RAYS (``mj_ray``, rangefinders, lidar): ``sim.ray(origin, direction)`` casts R rays per world -- ``origin`` / ``direction`` [N, R, 3] (or [R, 3]) in world coordinates, ``direction``
of any length -- and returns ``(dist [N, R] float32, geom [N, R] int32)``: the ray parameter of the nearest hit (metres for a unit direction) and the geom hit, -1.0 / -1 for none.
``sim.ray_sites(sites, local_dir)`` starts the rays at sites and skips each site's own body; ``sim.rangefinder()`` is [N, n_rangefinder], one reading per ``<rangefinder>`` of the MJCF
(along the site's +z, -1 for none or beyond the sensor's cutoff).  The rays see the body poses of the LAST launch -- ``outputs`` must name ``xpos`` and ``xquat`` (and ``site_xpos`` /
``site_xmat`` for the site variants) -- so exactly what ``MjData.geom_xpos`` holds then: exact after ``forward()``, one substep stale after ``step()``.  Three deviations from ``mj_ray``:
the rays see the COMPILED model's geoms, i.e. the collidable ones (visual geoms do not exist there); a mesh geom is its CONVEX HULL, the shape the engine collides with; there are no
geom groups.  A mesh geom whose only candidate pairs are with planes (or that has none) keeps no full hull in the compiled model: the ray calls raise a ``ValueError`` that names
it rather than cast through it.  The calls run a kernel of their own (grx_sim_ray / grx_sim_ray_sites) on torch's current stream and never synchronise; rays are not state.
``mesh="triangles"`` on ``ray``, ``ray_sites`` and ``rangefinder`` (default ``"hull"``) lifts the second deviation: a mesh geom is then the TRIANGLES of its file -- a ray passes the
gap of a gripper, the hole of a torus, and inside a room mesh it meets the walls -- with the same hit rule, two-sided (entry from outside, exit from inside).  The compiler keeps
every mesh geom's triangles and a bounding-volume hierarchy over them beside the packed model (``model.mesh_bvh``; ``save_model`` / ``load_model`` carry it), so a mesh needs no
hull to be seen and the ``ValueError`` above does not apply; the first such call uploads them once (``close()`` frees them), and the launch is the triangle variant of the ray
kernel (grx_sim_ray_tri, csrc/grx_trimesh.hip), in which a lane walks the hierarchy without a stack.  Any other value of ``mesh`` is a ``ValueError``.

    sim = grx.BatchedSim("maze_agent.xml", 4096, outputs=("xpos", "xquat", "site_xpos", "site_xmat"))
    fan = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros_like(ang)], dim=1)             # [64, 3] in the frame of the site "lidar"
    sim.step(nstep=5)
    dist, geom = sim.ray_sites("lidar", fan, max_dist=10.0)                                        # [N, 64]

CAMERAS (depth and segmentation): ``sim.render(cameras, height, width)`` returns ``depth [N, K, H, W]`` float32 for K ``<camera>`` elements of the MJCF (a name or a sequence of
names, at most 16 per call, 1 <= H, W <= 1024); ``segmentation=True`` returns ``(depth, seg)`` with ``seg`` int32 the id of the geom seen.  MuJoCo's conventions: a camera looks along
-z of its frame, +x right, +y up, row 0 is the top row, and the centre of pixel (r, c) has the camera-frame direction ``((2 (c + .5) / W - 1) tan(fovy / 2) W / H,
(1 - 2 (r + .5) / H) tan(fovy / 2), -1)``.  ``depth`` is the PLANAR depth, metres along the optical axis (the ray parameter along that direction); the Euclidean range is depth times
the direction's length.  No hit, or one deeper than a positive ``max_dist``: -1.0 / -1.  ``sim.render_pose(pos, xmat, fovy, height, width)`` is the same for cameras the caller
places (``pos`` [N, K, 3] or [K, 3], ``xmat`` [N, K, 9] or [K, 9] as ``site_xmat`` is, ``fovy`` a float or K of them).  ``exclude_own_body`` skips the geoms of each camera's body,
``exclude_body`` (one per camera, -1: none) those of another, ``include_static=False`` the world body's; ``mask`` renders only the worlds with a non-zero entry (the others read -1 in
fresh tensors and keep their bits in ``out=``).  A named camera sees the body poses of the LAST launch, as a ray does -- ``outputs`` must name ``xpos`` and ``xquat`` -- exact after
``forward()``, one substep stale after ``step()``.  ``sim.camera_id(name)`` is the row in ``model.info["camera"]`` (body, pose in the body's frame, fovy, mode, resolution; unnamed
cameras are ``_camera{k}``); ``sim.cameras_unserved`` maps the cameras whose ``mode`` is not ``fixed`` (``track*``, ``target*``) to the reason.  A kernel of its own (grx_sim_render): one
workgroup per image bins the geoms' bounding spheres to screen tiles once and each tile tests only what may touch it (``binning=False`` gives every tile every geom: the same image
bit for bit).  Deviations from MuJoCo's renderer: collidable geoms only, meshes as their convex hulls, no geom groups, no near-plane clipping (a surface 1 mm in front of the camera
is seen), no ``track`` / ``target`` modes.  ``mesh="triangles"`` on both render calls renders mesh geoms as their triangles instead (depth and segmentation; with ``rgb`` or
``normals`` it is a ``ValueError``: those shade hulls), through the render kernel's triangle variant (grx_sim_render_tri): the same stage, bin and trace, and at a mesh the 64
lanes of a tile walk the hierarchy together, a wave-wide vote deciding which nodes anyone needs; small hierarchies are copied to LDS once per image.

CAMERAS (colour and surface normals): ``rgb=True`` and ``normals=True`` of both render calls add a colour image and the surface normals; the result is then the tuple ``depth, [seg],
[rgb], [normal]`` in that fixed order (``out=`` takes the same tuple), and depth and seg are bit for bit what they are without the two keywords.  ``rgb`` is uint8 [N, K, H, W, 4],
bytes R, G, B, A -- packed RGBA8, not planar RGB: the kernel's lane is a pixel, so a packed pixel is ONE 32-bit store per lane and a tile row one 32-byte segment, where planar or
3-byte pixels would be byte stores; slice ``[..., :3]``.  A is 255 on a hit and 0 on a miss, which carries ``background``.  ``normal`` is float32 [N, K, H, W, 3]: the world-frame
OUTWARD unit normal of the geom's surface at the hit (outward also when seen from inside), 0 on a miss; where a surface has faces, the face the hit point x (geom frame) lies nearest
(plane +z; sphere x / |x|; capsule from the nearest point of its axis segment; ellipsoid (x / a^2, y / b^2, z / c^2) normalised; cylinder cap or side; box the face with the
smallest ||x_i| - s_i|; mesh, i.e. its hull, the plane with the smallest |n . x - c|).  The colour, in fp32 with d the pixel's direction: v = -d / |d|, s = ``ambient`` +
``diffuse`` |n . v|, plus ``sun_diffuse`` max(0, n_f . -sun) for a directional light travelling along the world-frame ``sun`` (n_f: n turned towards the viewer; ``sun=None``: none),
channel = floor(255 min(1, c s) + 0.5).  c is the geom's colour clamped to [0, 1]: ``colors``, a float32 device tensor [ngeom, 3], or [N, ngeom, 3] for each world its own colours
(visual domain randomisation); ``None``: ``model.info["geom_rgba"]``, which the compiler records per COMPILED geom -- the geom's own ``rgba`` through the default classes, else its
``<material>``'s, else MuJoCo's 0.5 0.5 0.5 1 -- uploaded once.  With ``mask``, the worlds left out read depth -1, the background with alpha 0 and normal 0 in fresh tensors.  A
kernel of its own again (grx_sim_render_rgb, csrc/grx_camera_rgb.hip): the depth kernel's stage, bin and trace, and a shade phase in which a wave walks the DISTINCT winners of its
tile, so that the normal's type switch stays wave-uniform.  This is a self-contained shading model, not MuJoCo's OpenGL renderer: no textures (a textured material counts with its
``rgba``), no transparency (alpha makes no geom transparent), no shadows, no specular term, no visual-only geoms, no mesh triangles (a mesh is shaded as its hull).

    sim = grx.BatchedSim("quadruped.xml", 4096, outputs=("xpos", "xquat"))
    sim.step(nstep=5)
    depth = sim.render("head_cam", 64, 64, exclude_own_body=True, max_dist=10.0)                   # [N, 1, 64, 64]
    depth, rgb = sim.render("head_cam", 64, 64, rgb=True, colors=my_rgb, sun=(0.3, -0.5, -0.8))    # rgb: uint8 [N, 1, 64, 64, 4]

INVERSE KINEMATICS: ``qpos, err, iters = sim.solve_ik(sites, target_pos, target_quat=None, qpos0=None, dofs=None, damping=1e-2, max_step=0.5, tol=1e-4, max_iters=32,
rot_weight=1.0, clamp_limits=True, mask=None, out=None)`` puts K = 1 .. 4 sites where the caller wants them: damped least squares over ``mj_jacSite``, the whole loop of a world in
one launch (grx_sim_ik: one wave per world, its own kinematics, so no output is needed and nothing of the step path is launched).  ``sim.qpos`` is never written; assign the
result if you want it.  Per world, with q = ``qpos0`` (default ``sim.qpos``):
  1. forward kinematics of the compiled tree at q (hinge, slide and free joints; free-joint quaternions normalised as ``mj_kinematics`` does; mocap bodies at ``sim.mocap_pos`` /
     ``sim.mocap_quat``);
  2. the error: ``e_pos,k = p*_k - p_k(q)`` and, with ``target_quat`` (w, x, y, z; need not be unit), ``d = r*_k (x) conj(r_k(q))``, negated if ``d.w < 0``, ``e_rot,k = rot_weight 2
     atan2(|d.v|, d.w) d.v / |d.v|`` (0 for ``|d.v| = 0``), a world-frame rotation vector; e stacks these per site, position first (m = 6 K components, or 3 K);
  3. stop if ``|e| < tol`` or ``max_iters`` updates have been made;
  4. J [m, nv]: the rows ``jacp_k`` and ``rot_weight jacr_k``; the columns of the dofs outside ``dofs`` (joint names, or a bool array [nv]) are zero;
  5. ``y = (J J' + damping^2 I)^-1 e`` by Cholesky, ``dq = J' y``, scaled to ``max_step`` if longer;
  6. ``q <- mj_integratePos(q, dq, 1)``; with ``clamp_limits`` every limited hinge or slide joint is clamped into ``jnt_range``.  Only coordinates whose dof is in ``dofs`` are written:
     the others come back bit for bit.  Go to 1.
``err`` [N] is ``|e|`` at the returned ``qpos`` [N, nq], ``iters`` [N] int32 the number of updates.  A masked-out world returns ``qpos0``, -1, 0; a world whose ``qpos0`` or targets are
not finite returns ``qpos0``, +inf, 0.  Wrong shapes, dtypes or parameters are a ``ValueError`` before the device is touched.

    qpos, err, iters = sim.solve_ik("grip", goal_xyz.view(4096, 1, 3), dofs=arm_joint_names)      # goal_xyz: [N, 3] float32 on the device
    sim.qpos.copy_(torch.where((err < 1e-3)[:, None], qpos, sim.qpos))
    sim.forward()

Not here: shape-specialised kernels for user models, split or cost-ordered launches, a handle in libgrx_env.so, keyframes, per-world geometry or poses,
equality-constraint forces in cfrc_ext, sensor reference frames and noise, MuJoCo's contact order, elliptic cones, rays against visual geoms, colour and normals on mesh triangles (mesh="triangles" serves rays, depth and segmentation), mesh files other than binary STL, geom groups, height fields, textures, shadows, specular light, transparency, visual-only geoms, tracking and targeting cameras, ball joints, nullspace posture terms, collision avoidance and per-site weights in solve_ik.
"""
import ctypes

import numpy as np

from .mjcf import CompiledModel, compile_mjcf

STATE = ("qpos", "qvel", "qacc_warmstart", "ctrl", "mocap_pos", "mocap_quat")
DYNAMICS = ("qM", "qfrc_smooth", "qacc_smooth", "qfrc_constraint", "qacc", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "site_jacp", "site_jacr")      # grx_sim_dynamics, in its order
JACOBIANS = ("site_jacp", "site_jacr")
OUTPUTS = ("xpos", "xquat", "site_xpos", "site_xmat", "site_xvelp", "site_xvelr", "sensordata", "ncon", "nefc") + DYNAMICS
PARAMS = ("gravity", "body_mass", "body_inertia", "dof_damping", "dof_armature", "dof_frictionloss", "jnt_stiffness", "jnt_springref", "jnt_range", "act_gear", "act_gainprm",
          "act_biasprm", "act_ctrlrange", "act_forcerange", "pair_friction", "pair_solref", "pair_solimp")      # include/grx_capi.h grx_sim_params_create
PARAM_BAD = dict(nonfinite=1, frictionloss=2, damping=4, inertial=8, armature=16, jnt_range=32, act_range=64)      # GRX_PARAM_BAD_*: the bits of params_invalid
CONTACTS = ("contact_geom", "contact_dim", "contact_efc_address", "contact_dist", "contact_pos", "contact_frame", "contact_force")      # grx_sim_contacts, in its order
_CONTACT_WIDTH = dict(contact_geom=(2,), contact_dim=(), contact_efc_address=(), contact_dist=(), contact_pos=(3,), contact_frame=(9,), contact_force=(6,))
_INT_TENSORS = ("ncon", "nefc", "contact_geom", "contact_dim", "contact_efc_address")
# The optional blocks in the order the C entries take them, and the entries from the one that takes every block down to the plain one: (the attribute that selects the entry,
# the entry, whether it takes the parameter object behind the handle, how many of _SIM_BLOCKS it takes).  A simulation calls the first entry whose attribute it has.
_SIM_BLOCKS = ("_dyn", "_con", "_frc", "_sns", "_wrn")
_SIM_ENTRIES = (("_wrn", "grx_sim_step_wrn", True, 5), ("_sns", "grx_sim_step_sns", True, 4), ("_frc", "grx_sim_step_frc", True, 3), ("_con", "grx_sim_step_con", True, 2), ("_p", "grx_sim_step_params", True, 1),
                ("_dyn", "grx_sim_step_dyn", False, 1), (None, "grx_sim_step", False, 0))
APPLIED = ("qfrc_applied", "xfrc_applied", "xipos")      # grx_sim_applied, in its order: two inputs the caller writes, one output
APPLIED_INPUTS = ("qfrc_applied", "xfrc_applied")
BODY_DYNAMICS = ("cfrc_ext", "cfrc_int", "cacc", "subtree_com")      # grx_sim_wrenches, in its order
# grx_sim_sensors: the type and object numbers of csrc/grx_sim_sensors.h, in its order
SENSOR_TYPES = ("jointpos", "jointvel", "actuatorpos", "actuatorvel", "actuatorfrc", "jointactuatorfrc", "framepos", "framequat", "framexaxis", "frameyaxis", "framezaxis",
                "framelinvel", "frameangvel", "velocimeter", "gyro", "framelinacc", "frameangacc", "accelerometer", "force", "torque")
SENSOR_OBJECTS = ("joint", "actuator", "site", "xbody")
_SENSOR_JOINT, _SENSOR_ACTUATOR, _SENSOR_SITE_ONLY = ("jointpos", "jointvel", "jointactuatorfrc"), ("actuatorpos", "actuatorvel", "actuatorfrc"), ("velocimeter", "gyro", "accelerometer", "force", "torque")
_SENSOR_WRENCH = ("force", "torque")      # read cfrc_int: served where body_dynamics names it
_SENSOR_NO_CUTOFF = ("framequat", "framexaxis", "frameyaxis", "framezaxis")
MAXJAC = 16      # GRX_SIM_MAXJAC: the site selection rides inside the launch's argument block
MAXCAM = 16      # GRX_CAM_MAX: the cameras of one render call ride there as well
MAXSIDE = 1024   # GRX_CAM_MAX_SIDE: largest image height / width


def _table_maxcon(req):
    """the contact-list capacity of a handle whose model requests `req` (csrc/grx_host_model.h: the request if it lies in 1 .. 64, else the default 32)"""
    return req if 0 < req <= 64 else 32


class _Params:
    """sim.params: one attribute per named table, the [N, ...] device tensor the caller writes"""

    def __repr__(self):
        return "params(" + ", ".join(f"{k}{tuple(v.shape)}" for k, v in self.__dict__.items()) + ")"


class BatchedSim:
    def __init__(self, model, num_worlds, device="cuda:0", capacity=None, overflow="rerun", outputs=(), compile_kwargs=None, jac_sites=None, model_params=(), contacts=(), applied=(), sensors=(),
                 body_dynamics=()):
        """model: path of an MJCF file, or a mjcf.CompiledModel.  capacity: dict(maxcon=, maxefc=, jpool=) of the tables the step launch runs on (None: the compiler's
        default, 32 contacts / 144 rows / 2 032 Jacobian words).  overflow: "rerun" -- a world that exceeds a table in some substep is left untouched by the step launch and run
        again, right behind it, on the large tables (core.RERUN_CAPACITY), so no contact is dropped; "flag" -- it goes on with the excess contacts dropped and the status bits
        CON_OVERFLOW / EFC_OVERFLOW say so.  outputs: the MjData fields to allocate and write, any of sim.OUTPUTS.  compile_kwargs: passed to compile_mjcf (touch_filter,
        keep_sites, mutate, ...).  jac_sites: the names of the sites whose Jacobians site_jacp / site_jacr hold, in the order of their rows (None: every site of the model, which must
        then have at most 16).  model_params: the tables that are per world, any of sim.PARAMS (module docstring).  contacts: the members of the contact list to allocate and write, any of sim.CONTACTS
        (module docstring).  applied: the applied-force inputs and xipos, any of sim.APPLIED (module docstring).  sensors: names of <sensor> children of the MJCF, or "all" (module docstring, SENSORS).  body_dynamics: the per-body
        outputs of mj_rnePostConstraint to allocate and write, any of sim.BODY_DYNAMICS (module docstring, BODY WRENCHES).  Nothing is allocated and no library is loaded before the first tensor is touched or the first launch: the name lookups work without a device."""
        if int(num_worlds) < 1:
            raise ValueError("num_worlds must be at least 1")
        if overflow not in ("rerun", "flag"):
            raise ValueError(f"overflow must be 'rerun' or 'flag', not {overflow!r}")
        if isinstance(outputs, str):
            outputs = (outputs,)
        unknown = [o for o in outputs if o not in OUTPUTS]
        if unknown:
            raise ValueError(f"unknown output(s) {unknown}; the optional outputs are {OUTPUTS}")
        if capacity is not None and not set(capacity) <= {"maxcon", "maxefc", "jpool"}:
            raise ValueError(f"capacity takes maxcon, maxefc and jpool, not {sorted(set(capacity) - {'maxcon', 'maxefc', 'jpool'})}")
        if isinstance(model_params, str):
            model_params = (model_params,)
        model_params = tuple(model_params)
        unknown = [p for p in model_params if p not in PARAMS]
        if unknown:
            raise ValueError(f"unknown model parameter(s) {unknown}; the per-world parameters are {PARAMS}")
        if len(set(model_params)) != len(model_params):
            raise ValueError(f"model_params names a parameter twice: {model_params}; the per-world parameters are {PARAMS}")
        self.param_names = tuple(p for p in PARAMS if p in model_params)
        if isinstance(contacts, str):
            contacts = (contacts,)
        contacts = tuple(contacts)
        unknown = [c for c in contacts if c not in CONTACTS]
        if unknown:
            raise ValueError(f"unknown contact output(s) {unknown}; the contact outputs are {CONTACTS}")
        if len(set(contacts)) != len(contacts):
            raise ValueError(f"contacts names an output twice: {contacts}; the contact outputs are {CONTACTS}")
        self.contacts = tuple(c for c in CONTACTS if c in contacts)
        if isinstance(applied, str):
            applied = (applied,)
        applied = tuple(applied)
        unknown = [a for a in applied if a not in APPLIED]
        if unknown:
            raise ValueError(f"unknown applied name(s) {unknown}; the applied-force tensors are {APPLIED}")
        if len(set(applied)) != len(applied):
            raise ValueError(f"applied names a tensor twice: {applied}; the applied-force tensors are {APPLIED}")
        self.applied = tuple(a for a in APPLIED if a in applied)
        if isinstance(body_dynamics, str):
            body_dynamics = (body_dynamics,)
        body_dynamics = tuple(body_dynamics)
        unknown = [a for a in body_dynamics if a not in BODY_DYNAMICS]
        if unknown:
            raise ValueError(f"unknown body_dynamics name(s) {unknown}; the per-body outputs are {BODY_DYNAMICS}")
        if len(set(body_dynamics)) != len(body_dynamics):
            raise ValueError(f"body_dynamics names an output twice: {body_dynamics}; the per-body outputs are {BODY_DYNAMICS}")
        self.body_dynamics = tuple(a for a in BODY_DYNAMICS if a in body_dynamics)
        kw = dict(compile_kwargs or {})
        if kw.get("origin") is not None or kw.get("shift_body") is not None:
            raise ValueError("BatchedSim returns raw engine coordinates: compile the model in the MJCF's own frame (no origin) and without a shift group")
        if isinstance(model, CompiledModel):
            if kw:
                raise ValueError("compile_kwargs apply to an MJCF path, not to a CompiledModel")
            self.model = model.with_capacity(**capacity) if capacity else model
        else:
            self.model = compile_mjcf(str(model), capacity=capacity, **kw)
        if self.model.origin.any():
            raise ValueError("BatchedSim needs a model compiled in the MJCF's own frame (origin 0)")
        m = self.model
        self.num_worlds, self.device_name, self.overflow = int(num_worlds), device, overflow
        self.outputs = tuple(o for o in OUTPUTS if o in outputs)
        self.nq, self.nv, self.nu, self.nbody, self.nsite, self.nmocap = (m.dim(k) for k in ("nq", "nv", "nu", "nbody", "nsite", "nmocap"))
        self.ntouch = len(np.asarray(m.tables.get("touch_body", [])).reshape(-1))
        self.timestep = m.opt("timestep")
        self.dynamics = tuple(o for o in self.outputs if o in DYNAMICS)
        wants_jac = any(o in JACOBIANS for o in self.outputs)
        if isinstance(jac_sites, str):
            jac_sites = (jac_sites,)
        if jac_sites is not None and not wants_jac:
            raise ValueError("jac_sites selects the rows of site_jacp / site_jacr, and neither is among the outputs")
        if jac_sites is None:      # every site, row = site id (a site without a name has a row all the same)
            if wants_jac and self.nsite > MAXJAC:
                raise ValueError(f"the model has {self.nsite} sites: name at most {MAXJAC} of them in jac_sites")
            by_id = {i: name for name, i in m.names.get("site", {}).items()}
            self._jac_ids = tuple(range(self.nsite)) if wants_jac else ()
            self.jac_sites = tuple(by_id.get(i) for i in self._jac_ids)
        else:
            self.jac_sites = tuple(jac_sites)
            if len(set(self.jac_sites)) != len(self.jac_sites):
                raise ValueError(f"jac_sites names a site twice: {self.jac_sites}")
            if len(self.jac_sites) > MAXJAC:
                raise ValueError(f"jac_sites names {len(self.jac_sites)} sites; a launch carries at most {MAXJAC}")
            self._jac_ids = tuple(self.site_id(name) for name in self.jac_sites)
        if wants_jac and not self._jac_ids:
            raise ValueError("site_jacp / site_jacr need at least one site (the model has none, or jac_sites is empty)")
        self._resolve_sensors(sensors)
        self._t = None      # the device tensors, made on first use
        self._h = self._h_big = self.lane = self._p = self._frc = self._sns = self._wrn = None

    # ------------------------------------------------------------------ names (CompiledModel.names / tables): no device needed
    def _lookup(self, kind, name):
        table = self.model.names.get(kind, {})
        if name not in table:
            raise KeyError(f"no {kind} named {name!r}; the compiled model's {kind} names are {sorted(table)}")
        return int(table[name])

    def body_id(self, name):
        """row of `name` in xpos / xquat: a body of the COMPILED model (a static child merged into its parent has no row of its own)"""
        return self._lookup("body", name)

    def site_id(self, name):
        return self._lookup("site", name)

    def geom_id(self, name):
        """id of the geom `name` as contact_geom holds it: a geom of the COMPILED model (the tables pair_geom1 / pair_geom2 index)"""
        return self._lookup("geom", name)

    @property
    def contact_capacity(self):
        """slots per world of the contact outputs: the contact-list capacity (maxcon) of the tables the step launch runs on, or -- when overflow="rerun" runs a world that
        exceeds them again on the large tables -- of those, so that a re-run world keeps all its contacts"""
        from .core import rerun_capacity

        big = rerun_capacity() if self.overflow == "rerun" else None
        return _table_maxcon(int(big["maxcon"]) if big else self.model.dim("maxcon_req"))

    def jac_row(self, name):
        """row of the site `name` in site_jacp / site_jacr (its position in jac_sites)"""
        self.site_id(name)
        if name not in self.jac_sites:
            raise KeyError(f"site {name!r} is not among jac_sites {self.jac_sites}")
        return self.jac_sites.index(name)

    # ------------------------------------------------------------------ sensors (module docstring, SENSORS): no device needed
    def _sensor_serve(self, name, rec):
        """(type, objtype, objid) of csrc/grx_sim_sensors.h for the row `rec` of model.info["sensor"], or ValueError with the reason it is not served"""
        m, kind, objtype, objname = self.model, rec["type"], rec["objtype"], rec["objname"]
        who = f"sensor {name!r} (<{kind}>)"
        if kind == "touch":
            raise ValueError(f"{who}: touch readings are served by outputs=('sensordata',) with compile_kwargs=dict(touch_filter=...)")
        if kind == "rangefinder":
            raise ValueError(f"{who}: rangefinders are served by sim.rangefinder()")
        if kind in _SENSOR_WRENCH and objtype != "site":
            raise ValueError(f"{who}: force and torque sensors read cfrc_int of a site's body and are attached to a site")
        if kind in _SENSOR_WRENCH and "cfrc_int" not in self.body_dynamics:
            raise ValueError(f"{who}: force and torque sensors need cfrc_int / cfrc_ext, which this simulation forms only on request: name 'cfrc_int' in body_dynamics=")
        if kind not in SENSOR_TYPES:
            raise ValueError(f"{who}: this type is not served; the served types are {SENSOR_TYPES}")
        if rec["reftype"] is not None:
            raise ValueError(f"{who}: a reference frame (reftype / refname) is not served; the reading would be in world coordinates")
        if kind in _SENSOR_JOINT:
            if objtype != "joint" or objname not in m.names["joint"]:
                raise ValueError(f"{who}: no joint named {objname!r} in the compiled model")
            j = int(m.names["joint"][objname])
            if int(np.asarray(m.tables["jnt_type"]).reshape(-1)[j]) < 2:
                raise ValueError(f"{who}: joint {objname!r} is a free or ball joint; the joint sensors read hinge and slide joints only")
            return SENSOR_TYPES.index(kind), SENSOR_OBJECTS.index("joint"), j
        if kind in _SENSOR_ACTUATOR:
            if objtype != "actuator" or objname not in m.names["actuator"]:
                raise ValueError(f"{who}: no actuator named {objname!r} in the compiled model")
            return SENSOR_TYPES.index(kind), SENSOR_OBJECTS.index("actuator"), int(m.names["actuator"][objname])
        if kind in _SENSOR_SITE_ONLY and objtype != "site":
            raise ValueError(f"{who}: this type is attached to a site")
        if objtype in ("body", "geom", "camera"):
            what = "the inertial frame of a body" if objtype == "body" else f"a {objtype}"
            raise ValueError(f"{who}: frame sensors on {what} are not served; use objtype='xbody' or a site at that frame")
        if objtype == "site":
            if objname not in m.names["site"]:
                raise ValueError(f"{who}: site {objname!r} is not among the compiled model's sites (keep_sites dropped it: compile_kwargs=dict(keep_sites=...))")
            return SENSOR_TYPES.index(kind), SENSOR_OBJECTS.index("site"), int(m.names["site"][objname])
        if objtype == "xbody":
            if objname not in m.names["body"]:
                raise ValueError(f"{who}: xbody {objname!r} has no row in the compiled model (the compiler merged it into its parent, or it does not exist): attach the sensor "
                                 "to a site on it -- sites keep their identity (compile_kwargs=dict(keep_sites=...) must keep it)")
            return SENSOR_TYPES.index(kind), SENSOR_OBJECTS.index("xbody"), int(m.names["body"][objname])
        raise ValueError(f"{who}: object type {objtype!r} is not served; frame sensors read a site or an xbody")

    def _resolve_sensors(self, sensors):
        rows, table = self.model.info.get("sensor", ()), self.model.names.get("sensor", {})
        self.sensors_unserved = {}
        if isinstance(sensors, str) and sensors == "all":
            picked = []
            for name, k in sorted(table.items(), key=lambda kv: kv[1]):
                try:
                    picked.append((name, self._sensor_serve(name, rows[k])))
                except ValueError as e:
                    self.sensors_unserved[name] = str(e)
        else:
            if isinstance(sensors, str):
                sensors = (sensors,)
            sensors = tuple(sensors)
            if len(set(sensors)) != len(sensors):
                raise ValueError(f"sensors names a sensor twice: {sensors}")
            unknown = [n for n in sensors if n not in table]
            if unknown:
                raise ValueError(f"no sensor(s) named {unknown} in the MJCF; its sensors are {sorted(table, key=table.get)}")
            picked = [(name, self._sensor_serve(name, rows[table[name]])) for name in sensors]
        self.sensors = tuple(name for name, _ in picked)
        self._sensor_spec, self._sensor_cut, self._sensor_adr, adr = [], [], {}, 0
        for name, (kind, obj, oid) in picked:
            dim = 4 if SENSOR_TYPES[kind] == "framequat" else (3 if kind >= SENSOR_TYPES.index("framepos") else 1)
            self._sensor_spec.append((kind, obj, oid, adr))
            self._sensor_cut.append(0.0 if SENSOR_TYPES[kind] in _SENSOR_NO_CUTOFF else max(float(rows[table[name]]["cutoff"]), 0.0))
            self._sensor_adr[name] = (adr, dim)
            adr += dim
        self.nsensordata = adr

    def sensor_adr(self, name):
        """(adr, dim): the columns [adr, adr + dim) of sensor_data that hold the sensor `name`"""
        if name not in self._sensor_adr:
            raise KeyError(f"sensor {name!r} is not among the requested sensors {self.sensors}: BatchedSim(..., sensors=...)")
        return self._sensor_adr[name]

    def sensor(self, name):
        """[N, dim] view of sensor_data: the reading of the sensor `name`"""
        adr, dim = self.sensor_adr(name)
        return self.sensor_data[:, adr:adr + dim]

    def actuator_id(self, name):
        return self._lookup("actuator", name)

    def mocap_id(self, name):
        """row of the mocap body `name` in mocap_pos / mocap_quat"""
        return self._lookup("mocap", name)

    def joint_qposadr(self, name):
        return int(np.asarray(self.model.tables["jnt_qposadr"]).reshape(-1)[self._lookup("joint", name)])

    def joint_dofadr(self, name):
        return int(np.asarray(self.model.tables["jnt_dofadr"]).reshape(-1)[self._lookup("joint", name)])

    def pair_ids(self, geom_a, geom_b=None):
        """rows of params.pair_friction / pair_solref / pair_solimp: the candidate pairs of the geom named geom_a (with geom_b: only those against that geom), ascending.
        Friction, solref and solimp are properties of the PAIR in the compiled model (the compiler has combined the two geoms' values)."""
        a = self._lookup("geom", geom_a)
        g1, g2 = (np.asarray(self.model.tables[k]).reshape(-1) for k in ("pair_geom1", "pair_geom2"))
        hit = (g1 == a) | (g2 == a)
        if geom_b is not None:
            b = self._lookup("geom", geom_b)
            hit &= (g1 == b) | (g2 == b)
        return [int(i) for i in np.nonzero(hit)[0]]

    def _param_shape(self, name):
        if name == "gravity":
            return (self.num_worlds, 3)
        shape = tuple(np.asarray(self.model.tables[name]).shape)
        while len(shape) > 1 and shape[-1] == 1:      # jnt_stiffness is stored [njnt, 1]
            shape = shape[:-1]
        return (self.num_worlds,) + shape

    # ------------------------------------------------------------------ device side
    def _shapes(self):
        n = self.num_worlds
        return dict(qpos=(n, self.nq), qvel=(n, self.nv), qacc_warmstart=(n, self.nv), ctrl=(n, self.nu), mocap_pos=(n, self.nmocap, 3), mocap_quat=(n, self.nmocap, 4),
                    xpos=(n, self.nbody, 3), xquat=(n, self.nbody, 4), site_xpos=(n, self.nsite, 3), site_xmat=(n, self.nsite, 9), site_xvelp=(n, self.nsite, 3),
                    site_xvelr=(n, self.nsite, 3), sensordata=(n, self.ntouch), ncon=(n,), nefc=(n,), qM=(n, self.nv, self.nv), site_jacp=(n, len(self._jac_ids), 3, self.nv),
                    site_jacr=(n, len(self._jac_ids), 3, self.nv), **{k: (n, self.nv) for k in DYNAMICS if k not in ("qM",) + JACOBIANS},
                    **{k: (n, self.contact_capacity) + _CONTACT_WIDTH[k] for k in CONTACTS},
                    qfrc_applied=(n, self.nv), xfrc_applied=(n, self.nbody, 6), xipos=(n, self.nbody, 3),
                    cfrc_ext=(n, self.nbody, 6), cfrc_int=(n, self.nbody, 6), cacc=(n, self.nbody, 6), subtree_com=(n, self.nbody, 3))

    def _ensure(self):
        if self._t is not None:
            return self._t
        import torch

        from . import _native
        from .core import OverflowLane, create_rerun_model

        self.device = torch.device(self.device_name)
        if self.device.type != "cuda":
            raise RuntimeError("BatchedSim runs on the GPU only (there is no CPU path)")
        self._L = _native.lib()
        dev_index = self.device.index or 0
        H, I, F = self.model.pack()
        self._h = _native.acquire_model(H, I, F, dev_index)
        self.lds_bytes = self._L.grx_model_lds_bytes(self._h)
        shapes = self._shapes()
        t = {}
        for k in STATE + self.outputs + self.contacts + self.applied + self.body_dynamics:
            t[k] = torch.zeros(shapes[k], dtype=torch.int32 if k in _INT_TENSORS else torch.float32, device=self.device)
        t["status_words"] = torch.zeros(self.num_worlds, dtype=torch.int32, device=self.device)
        tb = self.model.tables
        self._qpos0 = torch.from_numpy(np.asarray(tb["qpos0"], dtype=np.float32).reshape(-1)).to(self.device)
        self._mocap_pos0 = torch.from_numpy(np.asarray(tb.get("mocap_pos0", np.zeros(0)), dtype=np.float32).reshape(self.nmocap, 3)).to(self.device)
        self._mocap_quat0 = torch.from_numpy(np.asarray(tb.get("mocap_quat0", np.zeros(0)), dtype=np.float32).reshape(self.nmocap, 4)).to(self.device)
        self._t = t
        self._bufs = self._make_bufs(None)
        self._dyn = None
        if self.dynamics:      # one block for the step launch and for the re-run behind it
            self._dyn = _native.SimDynamicsStruct(**{k: t[k].data_ptr() for k in self.dynamics})
            if any(k in JACOBIANS for k in self.dynamics):
                self._dyn.njac = len(self._jac_ids)
                self._dyn.jac_site[:len(self._jac_ids)] = self._jac_ids
        self._con = None
        if self.contacts:      # again one block for both launches: ccap is the capacity of the larger handle
            self._con = _native.SimContactsStruct(ccap=self.contact_capacity, **{k[len("contact_"):]: t[k].data_ptr() for k in self.contacts})
        if self.applied:      # the fourth block, again one for both launches: a re-run world takes its applied rows along
            self._frc = _native.SimAppliedStruct(**{k: t[k].data_ptr() for k in self.applied})
        if self.sensors:      # the fifth block, one for both launches; the two host tables live as long as the simulation (each handle keeps a device copy, by content)
            t["sensor_data"] = torch.zeros((self.num_worlds, self.nsensordata), dtype=torch.float32, device=self.device)
            self._sns_host = (np.ascontiguousarray(self._sensor_spec, dtype=np.int32).reshape(-1, 4), np.ascontiguousarray(self._sensor_cut, dtype=np.float32))
            self._sns = _native.SimSensorsStruct(spec=self._sns_host[0].ctypes.data, cutoff=self._sns_host[1].ctypes.data, nsensor=len(self.sensors), ndata=self.nsensordata,
                                                 data=t["sensor_data"].data_ptr())
        if self.body_dynamics:      # the sixth block, one for both launches (a force / torque sensor is served only next to cfrc_int)
            self._wrn = _native.SimWrenchesStruct(**{k: t[k].data_ptr() for k in self.body_dynamics})
        if self.overflow == "rerun":
            self._h_big = create_rerun_model(self._L, self.model, dev_index, True)
            if self._h_big is not None:
                self.lane = OverflowLane(self.num_worlds, self.device, self.model, self._make_bufs, mode="entry")
        if self.param_names:      # one parameter object serves the handle of the step launch and that of the re-run
            from .env_capi import device_view

            names = (ctypes.c_char_p * len(self.param_names))(*[p.encode() for p in self.param_names])
            self._p = ctypes.c_void_p()
            _native.check(self._L.grx_sim_params_create(self._h, self._h_big, self.num_worlds, names, len(self.param_names), ctypes.byref(self._p)))
            self._params = _Params()
            for name in self.param_names:
                ptr, cnt = ctypes.c_void_p(), ctypes.c_int()
                _native.check(self._L.grx_sim_params_row(self._p, name.encode(), ctypes.byref(ptr), ctypes.byref(cnt)))
                shape = self._param_shape(name)
                assert int(np.prod(shape[1:])) == cnt.value, (name, shape, cnt.value)
                self._params.__dict__[name] = device_view(ptr.value, shape, np.float32, self.device)
            t["params_invalid"] = torch.zeros(self.num_worlds, dtype=torch.int32, device=self.device)
        # the C entry every launch calls and its fixed arguments: the first of _SIM_ENTRIES whose block this simulation has; it takes the blocks up to its own (None: not requested)
        _, name, takes_params, nblocks = next(e for e in _SIM_ENTRIES if e[0] is None or getattr(self, e[0]) is not None)
        self._entry = (getattr(self._L, name), (self._p,) if takes_params else (),
                       tuple(None if getattr(self, a) is None else ctypes.byref(getattr(self, a)) for a in _SIM_BLOCKS[:nblocks]))
        t["qpos"][:] = self._qpos0
        if self.nmocap:
            t["mocap_pos"][:], t["mocap_quat"][:] = self._mocap_pos0, self._mocap_quat0
        return t

    def __getattr__(self, name):      # the device tensors: sim.qpos ... sim.site_xpos; an output that was not requested does not exist
        if name.startswith("_"):
            raise AttributeError(name)
        if name in ("device", "lds_bytes"):      # known once the device side exists
            self._ensure()
            return self.__dict__[name]
        if name in STATE or name == "status_words" or name in self.__dict__.get("outputs", ()) or name in self.__dict__.get("contacts", ()) or name in self.__dict__.get("applied", ()) or name in self.__dict__.get("body_dynamics", ()):
            return self._ensure()[name]
        if name == "sensor_data":
            if not self.__dict__.get("sensors"):
                raise AttributeError("no sensor was requested: BatchedSim(..., sensors=...), names of the MJCF's <sensor> children or 'all'")
            return self._ensure()["sensor_data"]
        if name in ("params", "params_invalid"):
            if not self.__dict__.get("param_names"):
                raise AttributeError(f"no per-world parameters were named: BatchedSim(..., model_params=...), any of {PARAMS}")
            t = self._ensure()
            return t["params_invalid"] if name == "params_invalid" else self._params
        if name in OUTPUTS:
            raise AttributeError(f"output {name!r} was not requested: BatchedSim(..., outputs={self.__dict__.get('outputs', ())})")
        if name in APPLIED:
            raise AttributeError(f"{name!r} was not requested: BatchedSim(..., applied=...), any of {APPLIED}")
        if name in BODY_DYNAMICS:
            raise AttributeError(f"{name!r} was not requested: BatchedSim(..., body_dynamics=...), any of {BODY_DYNAMICS}")
        if name in CONTACTS:
            raise AttributeError(f"contact output {name!r} was not requested: BatchedSim(..., contacts={self.__dict__.get('contacts', ())})")
        raise AttributeError(name)

    def _make_bufs(self, mask):
        from . import _native

        t, b = self._t, _native.SimBuffersStruct()
        ptr = lambda x: x.data_ptr() if x.numel() else None
        b.qpos, b.qvel, b.qacc_ws = t["qpos"].data_ptr(), t["qvel"].data_ptr(), t["qacc_warmstart"].data_ptr()
        b.ctrl, b.mocap_pos, b.mocap_quat = ptr(t["ctrl"]), ptr(t["mocap_pos"]), ptr(t["mocap_quat"])
        for k in self.outputs:
            if k not in DYNAMICS:
                setattr(b, k, ptr(t[k]))
        b.status = t["status_words"].data_ptr()
        b.mask = None if mask is None else mask.data_ptr()
        return b

    def _mask(self, mask):
        if mask is None:
            return None
        import torch

        m = torch.as_tensor(mask, device=self.device)
        if m.shape != (self.num_worlds,):
            raise ValueError(f"mask must have shape ({self.num_worlds},), not {tuple(m.shape)}")
        return m.to(torch.uint8).contiguous()

    def _launch(self, nstep, forward_only, mask):
        import torch

        from . import _native
        from .core import stream_ptr

        self._ensure()
        if self._entry is None:
            raise RuntimeError("this BatchedSim is closed: its model handles and its parameter object are gone")
        m = self._mask(mask)
        self._mask_keep = m
        with torch.cuda.device(self.device):
            fn, head, blocks = self._entry
            go = lambda h: (lambda b: _native.check(fn(h, *head, ctypes.byref(b), *blocks, self.num_worlds, int(nstep), int(forward_only), stream_ptr(self.device))))
            self._bufs.mask = None if m is None else m.data_ptr()
            if self.lane is None:
                go(self._h)(self._bufs)
            else:      # entry mode: the step launch lists the worlds that exceed a table and leaves them untouched; the launch behind it runs them on the large tables
                self.lane.rerun_only(m, self._bufs, go(self._h), go(self._h_big))

    def step(self, nstep=1, mask=None):
        """mj_step(model, data, nstep) for every world (mask: only the worlds with a non-zero entry; the others keep state, outputs and status).  ctrl and the mocap poses are
        held over the substeps.  Enqueues on torch's current stream and returns nothing; the tensors are valid until the next launch."""
        if int(nstep) < 1:
            raise ValueError("nstep must be at least 1")
        self._launch(nstep, 0, mask)

    def forward(self, mask=None):
        """mj_forward: the derived fields of the state as given; qpos / qvel are left as they are, the warm start is updated"""
        self._launch(0, 1, mask)

    def commit_params(self, mask=None):
        """make the rows of sim.params take effect for the launches that follow (mask: only the worlds with a non-zero entry).  Each selected world's entry of
        params_invalid becomes 0, or the rules its row breaks (sim.PARAM_BAD); such a world keeps the parameters of its last good commit.  Enqueues on torch's current
        stream; never raises for a value, never synchronises."""
        import torch

        from . import _native
        from .core import stream_ptr

        if not self.param_names:
            raise RuntimeError("commit_params: no per-world parameters were named (BatchedSim(..., model_params=...))")
        t = self._ensure()
        m = self._mask(mask)
        self._commit_mask_keep = m
        with torch.cuda.device(self.device):
            _native.check(self._L.grx_sim_params_commit(self._p, None if m is None else m.data_ptr(), t["params_invalid"].data_ptr(), stream_ptr(self.device)))

    def reset(self, mask=None):
        """mj_resetData for the masked worlds (all by default): qpos0, zero velocities / warm start / ctrl / applied forces, the model's mocap poses; then forward().  The
        model parameters are not state: they stay as committed."""
        import torch

        t = self._ensure()
        m = self._mask(mask)
        sel = slice(None) if m is None else m.bool()
        t["qpos"][sel] = self._qpos0
        for k in ("qvel", "qacc_warmstart", "ctrl") + tuple(a for a in self.applied if a in APPLIED_INPUTS):
            t[k][sel] = 0.0
        if self.nmocap:
            t["mocap_pos"][sel], t["mocap_quat"][sel] = self._mocap_pos0, self._mocap_quat0
        self.forward(mask)

    # ------------------------------------------------------------------ rays (include/grx_capi.h grx_sim_ray / grx_sim_ray_sites; module docstring, RAYS)
    def _ray_need(self, what, needed, mesh="hull"):
        missing = [o for o in needed if o not in self.outputs]
        if missing:
            raise ValueError(f"{what} casts against the body poses of the last launch and needs the output(s) {missing}: BatchedSim(..., outputs={self.outputs + tuple(missing)})")
        if mesh == "triangles":      # a mesh needs no hull to be seen as triangles
            return
        tb = self.model.tables
        kind, hull = np.asarray(tb["geom_type"]).reshape(-1), np.asarray(tb["geom_hullnum"]).reshape(-1)
        bare = [int(g) for g in np.nonzero(kind == 7)[0] if g >= len(hull) or hull[g] < 4]
        if bare:      # the compiler keeps a mesh's full hull only for hull-vs-convex candidate pairs: a ray would pass through such a geom unseen
            by_id = {i: name for name, i in self.model.names.get("geom", {}).items()}
            raise ValueError(f"{what}: mesh geom(s) {[by_id.get(g, g) for g in bare]} have no full hull in the compiled model (a mesh keeps it only when it has a candidate pair with a "
                             "sphere, capsule, ellipsoid, cylinder, box or mesh geom; these meet planes only, or nothing), so rays cannot see them")

    @staticmethod
    def _mesh_kind(what, mesh, rgb=False, normals=False):
        """the mesh= keyword of the ray and render calls, checked without touching the device"""
        if mesh not in ("hull", "triangles"):
            raise ValueError(f'{what}: mesh is "hull" or "triangles", not {mesh!r}')
        if mesh == "triangles" and (rgb or normals):
            raise ValueError(f'{what}: mesh="triangles" serves depth and segmentation only; rgb=True and normals=True shade hulls (mesh="hull")')
        return mesh

    def _trimesh(self):
        """the triangle handle of this simulation's model (grx_sim_trimesh_create): made on the first call with mesh="triangles", one blocking upload, freed by close()"""
        from . import _native

        if self.__dict__.get("_tri") is None:
            self._ensure()
            bvh = self.model.mesh_bvh
            ngeom = int(self.model.dim("ngeom"))
            if bvh is None:
                if (np.asarray(self.model.tables["geom_type"]).reshape(-1) == 7).any():
                    raise ValueError('mesh="triangles": the model has mesh geoms but carries no triangles (it was saved before the compiler kept them): compile it again')
                bvh = dict(nodes=np.zeros((0, 8), np.int32), tris=np.zeros((0, 9), np.float32), geom_adr=-np.ones((ngeom, 2), np.int32))
            nodes, tris, adr = (np.ascontiguousarray(bvh[k], dtype=dt) for k, dt in (("nodes", np.int32), ("tris", np.float32), ("geom_adr", np.int32)))
            h = ctypes.c_void_p()
            _native.check(self._L.grx_sim_trimesh_create(self._h, nodes.ctypes.data, len(nodes), tris.ctypes.data, len(tris), adr.ctypes.data, len(adr), ctypes.byref(h)))
            self._tri = h
        return self._tri

    def _ray_exclude(self, exclude_body, n_rays):
        """[R] int32 device tensor of compiled body ids (-1: none), or None"""
        import torch

        if exclude_body is None:
            return None
        if isinstance(exclude_body, str):
            exclude_body = self.body_id(exclude_body)
        if isinstance(exclude_body, (int, np.integer)):
            exclude_body = [int(exclude_body)] * n_rays
        if not torch.is_tensor(exclude_body):
            exclude_body = [self.body_id(b) if isinstance(b, str) else int(b) for b in exclude_body]
        e = torch.as_tensor(exclude_body, device=self.device).to(torch.int32).contiguous()
        if e.shape != (n_rays,):
            raise ValueError(f"exclude_body must be one body or have length {n_rays}, not shape {tuple(e.shape)}")
        return e

    def _ray_out(self, out, n_rays):
        import torch

        if out is None:      # fresh tensors start as "no hit": with a mask the rows of the worlds it leaves out read -1.0 / -1
            return (torch.full((self.num_worlds, n_rays), -1.0, dtype=torch.float32, device=self.device), torch.full((self.num_worlds, n_rays), -1, dtype=torch.int32, device=self.device))
        dist, geom = out
        for x, dt in ((dist, torch.float32), (geom, torch.int32)):
            if x.shape != (self.num_worlds, n_rays) or x.dtype != dt or x.device != self.device or not x.is_contiguous():
                raise ValueError(f"out= takes a contiguous float32 and an int32 tensor of shape ({self.num_worlds}, {n_rays}) on {self.device}")
        return dist, geom

    def _ray_launch(self, fn, block, n_rays, keep, mesh="hull"):
        """fn: "grx_sim_ray" or "grx_sim_ray_sites"; mesh="triangles" launches its _tri variant with the triangle handle"""
        import torch

        from . import _native
        from .core import stream_ptr

        self._ray_keep = keep      # the inputs stay alive until the next ray call has replaced them (the launch is only enqueued)
        tri = (self._trimesh(),) if mesh == "triangles" else ()
        with torch.cuda.device(self.device):
            _native.check(getattr(self._L, fn + ("_tri" if tri else ""))(self._h, ctypes.byref(block), *tri, self.num_worlds, int(n_rays), stream_ptr(self.device)))

    def ray(self, origin, direction, exclude_body=None, max_dist=0.0, include_static=True, mask=None, out=None, mesh="hull"):
        """mj_ray for R rays in every world: origin, direction [N, R, 3] device tensors in world coordinates ([R, 3]: the same rays in every world); direction need not be unit.
        Returns (dist [N, R] float32, geom [N, R] int32): the parameter t of the nearest hit (metres for a unit direction) and the id of the geom hit (sim.geom_id), or -1.0 / -1
        for no hit, a hit beyond max_dist (when positive), a zero or non-finite direction.  exclude_body: a body name or compiled body id, or a list / tensor of R of them (-1:
        none): that body's geoms are skipped (mj_ray's bodyexclude).  include_static=False skips the geoms of the world body.  mask: only the worlds with a non-zero entry are
        written; the rows of the others read -1.0 / -1 in fresh tensors and keep their bits in out= tensors.  out=(dist, geom): write into these tensors.  Casts against the xpos / xquat of the LAST launch (exact after forward(), one substep stale after step()).
        Enqueues on torch's current stream; never synchronises.  mesh="triangles": a mesh geom is the triangles of its file and not its convex hull (module docstring, RAYS);
        the first such call uploads them."""
        import torch

        from . import _native

        self._ray_need("ray()", ("xpos", "xquat"), self._mesh_kind("ray()", mesh))
        t = self._ensure()
        o, d = (torch.as_tensor(x, device=self.device).to(torch.float32) for x in (origin, direction))
        if o.dim() == 2 and d.dim() == 3:
            o = o.expand(d.shape)
        if d.dim() == 2:
            d = d.expand((self.num_worlds,) + tuple(d.shape)) if o.dim() == 2 else d.expand(o.shape)
        if o.dim() == 2:
            o = o.expand((self.num_worlds,) + tuple(o.shape))
        if o.dim() != 3 or o.shape != d.shape or o.shape[0] != self.num_worlds or o.shape[2] != 3 or o.shape[1] < 1:
            raise ValueError(f"origin and direction must have shape ({self.num_worlds}, R, 3) or (R, 3), not {tuple(o.shape)} and {tuple(d.shape)}")
        o, d = o.contiguous(), d.contiguous()
        n_rays = o.shape[1]
        e, m = self._ray_exclude(exclude_body, n_rays), self._mask(mask)
        dist, geom = self._ray_out(out, n_rays)
        b = _native.SimRaysStruct(xpos=t["xpos"].data_ptr(), xquat=t["xquat"].data_ptr(), origin=o.data_ptr(), direction=d.data_ptr(), exclude_body=None if e is None else e.data_ptr(),
                                  mask=None if m is None else m.data_ptr(), dist=dist.data_ptr(), geom=geom.data_ptr(), max_dist=float(max_dist), include_static=int(bool(include_static)))
        self._ray_launch("grx_sim_ray", b, n_rays, (o, d, e, m), mesh)
        return dist, geom

    def ray_sites(self, sites, local_dir, exclude_own_body=True, exclude_body=None, max_dist=0.0, include_static=True, mask=None, out=None, mesh="hull"):
        """R rays that start at sites: ray r starts at site sites[r] (a name or id; one name: every ray) and runs along local_dir[r] ([R, 3], in the site's frame), in every
        world.  exclude_own_body: the geoms of the site's body are skipped (the rangefinder rule); the other arguments and the result are those of ray().  Reads site_xpos /
        site_xmat of the last launch as well.  The first call with a list of sites the model handle has not seen uploads it (one blocking copy; the handle keeps the 64 most recent
        lists); every later call with that list only enqueues.  mesh: as in ray()."""
        import torch

        from . import _native

        self._ray_need("ray_sites()", ("xpos", "xquat", "site_xpos", "site_xmat"), self._mesh_kind("ray_sites()", mesh))
        t = self._ensure()
        l = torch.as_tensor(local_dir, device=self.device).to(torch.float32).contiguous()
        if l.dim() != 2 or l.shape[1] != 3 or l.shape[0] < 1:
            raise ValueError(f"local_dir must have shape (R, 3), not {tuple(l.shape)}")
        n_rays = l.shape[0]
        if isinstance(sites, (str, int, np.integer)):
            sites = [sites] * n_rays
        ids = [self.site_id(s) if isinstance(s, str) else int(s) for s in sites]
        if len(ids) != n_rays:
            raise ValueError(f"sites names {len(ids)} sites for {n_rays} directions")
        bad = [s for s in ids if not 0 <= s < self.nsite]
        if bad:
            raise ValueError(f"site id(s) {bad} outside [0, {self.nsite})")
        host = (ctypes.c_int * n_rays)(*ids)
        e, m = self._ray_exclude(exclude_body, n_rays), self._mask(mask)
        dist, geom = self._ray_out(out, n_rays)
        b = _native.SimRaysStruct(xpos=t["xpos"].data_ptr(), xquat=t["xquat"].data_ptr(), site_xpos=t["site_xpos"].data_ptr(), site_xmat=t["site_xmat"].data_ptr(),
                                  ray_site=ctypes.cast(host, ctypes.c_void_p), local_dir=l.data_ptr(), exclude_body=None if e is None else e.data_ptr(),
                                  mask=None if m is None else m.data_ptr(), dist=dist.data_ptr(), geom=geom.data_ptr(), max_dist=float(max_dist), include_static=int(bool(include_static)),
                                  exclude_site_body=int(bool(exclude_own_body)))
        self._ray_launch("grx_sim_ray_sites", b, n_rays, (l, e, m, host), mesh)
        return dist, geom

    @property
    def n_rangefinder(self):
        return len(self.model.info.get("rangefinder", ()))

    def rangefinder_id(self, name):
        """column of the <rangefinder> sensor `name` in rangefinder()"""
        return self._lookup("rangefinder", name)

    def rangefinder(self, mask=None, mesh="hull"):
        """[N, n_rangefinder] float32: the reading of every <rangefinder> sensor of the MJCF, in sensor order -- the distance along the +z axis of the sensor's site to the
        nearest geom that does not belong to the site's body, -1 for none or for one beyond the sensor's positive cutoff (mjSENS_RANGEFINDER, over the geoms ray() sees).
        mask: the rows of the worlds it leaves out read -1.  mesh: as in ray()."""
        import torch

        self._mesh_kind("rangefinder()", mesh)
        rows = self.model.info.get("rangefinder", ())
        if not rows:
            raise ValueError("the model has no <rangefinder> sensor")
        lost = [name for name, k in self.model.names["rangefinder"].items() if rows[k]["site"] not in self.model.names["site"]]
        if lost:
            raise ValueError(f"the site of rangefinder(s) {sorted(lost)} is not among the model's sites (the sensor names none, or keep_sites dropped it: compile_kwargs=dict(keep_sites=...))")
        self._ray_need("rangefinder()", ("xpos", "xquat", "site_xpos", "site_xmat"), mesh)
        self._ensure()
        if self.__dict__.get("_rf") is None:
            self._rf = (torch.tensor([[0.0, 0.0, 1.0]] * len(rows), device=self.device), torch.tensor([[max(float(r["cutoff"]), 0.0) for r in rows]], dtype=torch.float32, device=self.device))
        z, cut = self._rf
        dist, _ = self.ray_sites([r["site"] for r in rows], z, exclude_own_body=True, mask=mask, mesh=mesh)
        beyond = (cut > 0) & (dist > cut)      # each sensor's own cutoff
        if mask is not None:
            beyond &= self._mask(mask).bool()[:, None]
        return dist.masked_fill_(beyond, -1.0)

    # ------------------------------------------------------------------ cameras (include/grx_capi.h grx_sim_render; module docstring, CAMERAS)
    def camera_id(self, name):
        """row of the <camera> `name` in model.info["camera"]"""
        return self._lookup("camera", name)

    @property
    def cameras_unserved(self):
        """name -> reason for the MJCF's cameras render() does not serve: the ones whose mode is not `fixed`"""
        rows = self.model.info.get("camera", ())
        return {name: f'mode="{rows[k]["mode"]}": render() serves fixed cameras only (a tracking or targeting camera turns with the scene; place it with render_pose())'
                for name, k in self.model.names.get("camera", {}).items() if rows[k]["mode"] != "fixed"}

    def _shade(self, what, rgb, normals, colors, ambient, diffuse, sun, sun_diffuse, background):
        """the shading keywords of both render calls, checked without touching the device: None when neither rgb nor normals is set, else the host half of the shade block"""
        if not (rgb or normals):
            return None
        ngeom = int(self.model.dim("ngeom"))
        if colors is not None and (not hasattr(colors, "shape") or tuple(colors.shape) not in ((ngeom, 3), (self.num_worlds, ngeom, 3))):
            raise ValueError(f"{what}: colors is a tensor of shape ({ngeom}, 3) or ({self.num_worlds}, {ngeom}, 3), not {tuple(getattr(colors, 'shape', ())) or type(colors).__name__}")
        if colors is None and rgb and len(self.model.info.get("geom_rgba", ())) != ngeom:
            raise ValueError(f'{what}: the model carries no info["geom_rgba"] (it was saved before the compiler recorded colours): compile it again or pass colors=')
        terms = [float(ambient), float(diffuse), float(sun_diffuse)]
        if not all(0.0 <= x < float("inf") for x in terms):
            raise ValueError(f"{what}: ambient, diffuse and sun_diffuse must be finite and >= 0, not {terms}")
        background = [float(x) for x in np.asarray(background, dtype=np.float64).reshape(-1)]
        if len(background) != 3 or not np.isfinite(background).all():
            raise ValueError(f"{what}: background is three finite values, not {background}")
        if sun is not None:
            sun = [float(x) for x in np.asarray(sun, dtype=np.float64).reshape(-1)]
            if len(sun) != 3 or not np.isfinite(sun).all() or not np.linalg.norm(sun) > 1e-10:
                raise ValueError(f"{what}: sun is a non-zero finite direction [3], not {sun}")
        level = np.floor(np.float32(255.0) * np.clip(np.asarray(background, dtype=np.float32), 0.0, 1.0) + np.float32(0.5)).astype(np.uint8)      # the kernel's rounding
        return dict(ambient=terms[0], diffuse=terms[1], sun=sun or [0.0, 0.0, 0.0], sun_diffuse=terms[2] if sun is not None else 0.0, background=background,
                    word=int(level[0]) | int(level[1]) << 8 | int(level[2]) << 16)      # the packed pixel of a miss: bytes R, G, B and alpha 0

    def _render(self, what, n_cams, height, width, fovy, segmentation, exclude_body, max_dist, include_static, mask, out, binning, tile, fill, rgb=False, normals=False, colors=None, shade=None, mesh="hull"):
        """the checks and the launch both render calls share; fill(block, t) -> what to keep alive: sets the block's camera poses once the device tensors exist.  shade: what
        _shade() returned; with it the launch is grx_sim_render_rgb and the result the tuple depth, [seg], [rgb], [normal]"""
        import torch

        from . import _native
        from .core import stream_ptr

        if not 1 <= n_cams <= MAXCAM:
            raise ValueError(f"{what} takes 1 .. {MAXCAM} cameras per call, not {n_cams}")
        height, width = int(height), int(width)
        if not (1 <= height <= MAXSIDE and 1 <= width <= MAXSIDE):
            raise ValueError(f"{what}: height x width = {height} x {width} is outside 1 .. {MAXSIDE}")
        if tile not in (None, "16x4", "8x8"):
            raise ValueError(f'{what}: tile is "16x4" or "8x8", not {tile!r}')
        fovy = [float(fovy)] * n_cams if isinstance(fovy, (int, float, np.floating, np.integer)) else [float(f) for f in fovy]
        if len(fovy) != n_cams or not all(0.0 < f < 180.0 for f in fovy):
            raise ValueError(f"{what}: fovy is one angle or {n_cams} of them, in degrees inside (0, 180), not {fovy}")
        if exclude_body is None:
            exclude = [-1] * n_cams
        elif isinstance(exclude_body, (str, int, np.integer)):
            exclude = [exclude_body] * n_cams
        else:
            exclude = list(exclude_body)
        exclude = [self.body_id(b) if isinstance(b, str) else int(b) for b in exclude]
        if len(exclude) != n_cams:
            raise ValueError(f"{what}: exclude_body must be one body or name {n_cams} of them (-1: none), not {len(exclude)}")
        self._ray_need(what, ("xpos", "xquat"), mesh)
        t = self._ensure()
        m = self._mask(mask)
        shape = (self.num_worlds, n_cams, height, width)
        rgb, normals = bool(rgb) and shade is not None, bool(normals) and shade is not None
        # the images of the call in the order of its result: (wanted, trailing shape, dtype, what a fresh tensor starts as -- "no hit", which the masked-out worlds then read)
        kinds = ((True, (), torch.float32, -1.0), (segmentation, (), torch.int32, -1), (rgb, (4,), torch.uint8, None), (normals, (3,), torch.float32, 0.0))
        wanted = [k for k in kinds if k[0]]
        if out is None:
            images = [torch.full(shape + tail, 0 if start is None else start, dtype=dt, device=self.device) for _, tail, dt, start in wanted]
            if rgb:      # the background colour, alpha 0: a fill of the packed words, no copy from the host
                images[1 + bool(segmentation)].view(torch.int32).fill_(shade["word"])
        else:
            images = [out] if len(wanted) == 1 else list(out)
            if len(images) != len(wanted) or any(not torch.is_tensor(x) or x.shape != shape + tail or x.dtype != dt or x.device != self.device or not x.is_contiguous()
                                                 for x, (_, tail, dt, _) in zip(images, wanted)):
                if shade is None:
                    raise ValueError(f"out= takes a contiguous float32 tensor{' and an int32 tensor' if segmentation else ''} of shape {shape} on {self.device}")
                raise ValueError(f"out= takes contiguous tensors on {self.device} in the order of the result: " + ", ".join(f"{str(dt).split('.')[-1]} {shape + tail}" for _, tail, dt, _ in wanted))
        it = iter(images)
        depth, seg, rgba, normal = (next(it) if k[0] else None for k in kinds)
        if rgba is not None and rgba.data_ptr() % 4:
            raise ValueError("out=: the rgb tensor must start at a 4-byte boundary (a pixel is stored as one 32-bit word)")
        host = ((ctypes.c_float * n_cams)(*fovy), (ctypes.c_int * n_cams)(*exclude))
        b = _native.SimCamerasStruct(xpos=t["xpos"].data_ptr(), xquat=t["xquat"].data_ptr(), cam_fovy=ctypes.cast(host[0], ctypes.c_void_p), exclude_body=ctypes.cast(host[1], ctypes.c_void_p),
                                     mask=None if m is None else m.data_ptr(), depth=depth.data_ptr(), seg=None if seg is None else seg.data_ptr(), max_dist=float(max_dist),
                                     include_static=int(bool(include_static)), no_binning=int(not binning), tile_16x4=int(tile == "16x4"))
        if shade is None:
            self._ray_keep = (fill(b, t), m, host)      # alive until the next ray or camera call has replaced them (the launch is only enqueued)
            with torch.cuda.device(self.device):
                if mesh == "triangles":
                    _native.check(self._L.grx_sim_render_tri(self._h, ctypes.byref(b), self._trimesh(), self.num_worlds, n_cams, height, width, stream_ptr(self.device)))
                else:
                    _native.check(self._L.grx_sim_render(self._h, ctypes.byref(b), self.num_worlds, n_cams, height, width, stream_ptr(self.device)))
            return (depth, seg) if segmentation else depth
        if colors is None and rgb:      # the compiler's table, uploaded once per simulation
            if self.__dict__.get("_geom_rgb") is None:
                self._geom_rgb = torch.tensor(np.asarray(self.model.info["geom_rgba"], dtype=np.float64).reshape(-1, 4)[:, :3], dtype=torch.float32, device=self.device).contiguous()
            colors = self._geom_rgb
        elif colors is not None:
            colors = torch.as_tensor(colors, device=self.device).to(torch.float32).contiguous()
        s = _native.SimShadeStruct(rgba=None if rgba is None else rgba.data_ptr(), normal=None if normal is None else normal.data_ptr(), colors=None if colors is None else colors.data_ptr(),
                                   colors_per_world=int(colors is not None and colors.dim() == 3), ambient=shade["ambient"], diffuse=shade["diffuse"],
                                   sun=(ctypes.c_float * 3)(*shade["sun"]), sun_diffuse=shade["sun_diffuse"], background=(ctypes.c_float * 3)(*shade["background"]))
        self._ray_keep = (fill(b, t), m, host, colors)
        with torch.cuda.device(self.device):
            _native.check(self._L.grx_sim_render_rgb(self._h, ctypes.byref(b), ctypes.byref(s), self.num_worlds, n_cams, height, width, stream_ptr(self.device)))
        return tuple(images)

    def render(self, cameras, height, width, segmentation=False, exclude_own_body=False, exclude_body=None, max_dist=0.0, include_static=True, mask=None, out=None, binning=True, tile=None,
               rgb=False, normals=False, colors=None, ambient=0.3, diffuse=0.7, sun=None, sun_diffuse=0.5, background=(0.0, 0.0, 0.0), mesh="hull"):
        """Depth images of the MJCF's cameras: `cameras` a <camera> name or a sequence of K of them (at most 16 per call).  Returns depth [N, K, height, width] float32, the planar
        depth in metres along each camera's optical axis (module docstring, CAMERAS); with segmentation=True (depth, seg), seg int32 the id of the geom seen (sim.geom_id).  No
        hit, or one deeper than max_dist (when positive): -1.0 / -1.  exclude_own_body skips the geoms of each camera's body, exclude_body (one body or K, names or ids, -1:
        none) those of another; include_static=False the world body's.  mask: only the worlds with a non-zero entry are rendered; the images of the others read -1 in fresh
        tensors and keep their bits in out= (a depth tensor, or (depth, seg) with segmentation).  binning=False gives every screen tile every geom and tile="16x4" traces wide
        tiles instead of 8 x 8: the same image bit for bit, for A/B timing.  Sees the xpos / xquat of the LAST launch (exact after forward(), one substep stale after step()).  Enqueues on
        torch's current stream; never synchronises.
        rgb=True adds a colour image, normals=True the surface normals: the result is then the tuple depth, [seg], [rgb], [normal] in that fixed order, and out= takes the same
        tuple.  rgb is uint8 [N, K, height, width, 4], bytes R, G, B, A: PACKED RGBA8 and not planar RGB, because the kernel's lane is a pixel and a packed pixel is one 32-bit
        store per lane (a tile row of 8 pixels one 32-byte segment), where planar or 3-byte pixels would be byte stores; slice [..., :3] for RGB.  A is 255 on a hit, 0 on a miss,
        and a miss carries `background`.  normal is float32 [N, K, height, width, 3], the world-frame outward unit normal at the hit, 0 on a miss.  colors: a float32 device tensor
        [ngeom, 3], or [N, ngeom, 3] for per-world colours, in 0 .. 1; None: the MJCF's (model.info["geom_rgba"], uploaded once).  The shading (module docstring, CAMERAS):
        ambient + diffuse |n . v| towards the viewer, plus sun_diffuse max(0, n_f . -sun) for a directional light that travels along the world-frame `sun` (None: no sun).  In
        fresh tensors the worlds `mask` leaves out read depth -1, the background with alpha 0 and normal 0.
        mesh="triangles": depth and segmentation see a mesh geom as the triangles of its file and not as its convex hull (module docstring, CAMERAS); not with rgb or normals."""
        self._mesh_kind("render()", mesh, rgb, normals)
        shade = self._shade("render()", rgb, normals, colors, ambient, diffuse, sun, sun_diffuse, background)
        names = [cameras] if isinstance(cameras, str) else list(cameras)
        rows = [self.model.info["camera"][self.camera_id(n)] for n in names]
        unserved = self.cameras_unserved
        for n in names:
            if n in unserved:
                raise ValueError(f"camera {n!r}: {unserved[n]}")

        def fill(b, t):
            host = ((ctypes.c_int * len(rows))(*[r["body"] for r in rows]), (ctypes.c_float * (3 * len(rows)))(*[x for r in rows for x in r["pos"]]),
                    (ctypes.c_float * (4 * len(rows)))(*[x for r in rows for x in r["quat"]]))
            b.cam_body, b.cam_pos, b.cam_quat = (ctypes.cast(h, ctypes.c_void_p) for h in host)
            b.exclude_own_body = int(bool(exclude_own_body))
            return host

        return self._render("render()", len(rows), height, width, [r["fovy"] for r in rows], segmentation, exclude_body, max_dist, include_static, mask, out, binning, tile, fill,
                            rgb, normals, colors, shade, mesh)

    def render_pose(self, pos, xmat, fovy, height, width, segmentation=False, exclude_body=None, max_dist=0.0, include_static=True, mask=None, out=None, binning=True, tile=None,
                    rgb=False, normals=False, colors=None, ambient=0.3, diffuse=0.7, sun=None, sun_diffuse=0.5, background=(0.0, 0.0, 0.0), mesh="hull"):
        """render() for cameras the caller places: pos [N, K, 3] or [K, 3] (the same cameras in every world), xmat [N, K, 9] or [K, 9] the camera frames' rotations (camera ->
        world, row-major as site_xmat is: the columns are the camera's right, up and backward axes), fovy one angle or K in degrees.  The other arguments and the result are
        those of render(); there is no body of its own to exclude."""
        import torch

        self._mesh_kind("render_pose()", mesh, rgb, normals)
        shade = self._shade("render_pose()", rgb, normals, colors, ambient, diffuse, sun, sun_diffuse, background)
        self._ray_need("render_pose()", ("xpos", "xquat"), mesh)
        self._ensure()
        p, x = (torch.as_tensor(v, device=self.device).to(torch.float32) for v in (pos, xmat))
        if p.dim() == 2:
            p = p.expand((self.num_worlds,) + tuple(p.shape))
        if x.dim() == 2:
            x = x.expand((self.num_worlds,) + tuple(x.shape))
        if p.dim() != 3 or x.dim() != 3 or p.shape[0] != self.num_worlds or p.shape[2] != 3 or x.shape != (self.num_worlds, p.shape[1], 9):
            raise ValueError(f"pos must have shape ({self.num_worlds}, K, 3) or (K, 3) and xmat ({self.num_worlds}, K, 9) or (K, 9), not {tuple(p.shape)} and {tuple(x.shape)}")
        p, x = p.contiguous(), x.contiguous()

        def fill(b, t):
            b.pose_pos, b.pose_mat = p.data_ptr(), x.data_ptr()
            return (p, x)

        return self._render("render_pose()", int(p.shape[1]), height, width, fovy, segmentation, exclude_body, max_dist, include_static, mask, out, binning, tile, fill,
                            rgb, normals, colors, shade, mesh)

    # ------------------------------------------------------------------ inverse kinematics (include/grx_capi.h grx_sim_ik; module docstring, INVERSE KINEMATICS)
    def _ik_dofs(self, dofs):
        """[nv] uint8 host array of the dofs a solve_ik call may move, or None for all of them"""
        if dofs is None:
            return None
        if isinstance(dofs, str):
            dofs = (dofs,)
        if len(dofs) and all(isinstance(d, str) for d in dofs):
            sel = np.zeros(self.nv, np.uint8)
            kind = np.asarray(self.model.tables["jnt_type"]).reshape(-1)
            for name in dofs:
                a = self.joint_dofadr(name)
                sel[a: a + (6 if kind[self._lookup("joint", name)] == 0 else 1)] = 1
            return sel
        sel = np.asarray(dofs)
        if sel.dtype != np.bool_ or sel.shape != (self.nv,):
            raise ValueError(f"dofs is None, a sequence of joint names or a bool array of shape ({self.nv},)")
        return np.ascontiguousarray(sel, dtype=np.uint8)

    def solve_ik(self, sites, target_pos, target_quat=None, qpos0=None, dofs=None, damping=1e-2, max_step=0.5, tol=1e-4, max_iters=32, rot_weight=1.0, clamp_limits=True,
                 mask=None, out=None):
        """Damped-least-squares inverse kinematics for every world, the whole loop in one launch (module docstring, INVERSE KINEMATICS): moves the K = 1 .. 4 named sites
        to target_pos [N, K, 3] ([K, 3]: the same targets in every world) and, when given, target_quat [N, K, 4] (w, x, y, z; need not be unit), starting at qpos0 [N, nq]
        (default sim.qpos, which is never written).  dofs: the joints (names) or dofs (bool [nv]) the solve may move; the coordinates of the others come back bit for bit.
        Returns (qpos [N, nq] float32, err [N] float32: the error norm at that qpos, iters [N] int32: the updates made).  A masked-out world returns qpos0, -1, 0; a world with a
        non-finite qpos0 or target returns qpos0, +inf, 0.  out=(qpos, err, iters): write into these tensors.  Enqueues on torch's current stream; never synchronises."""
        import torch

        from . import _native
        from .core import stream_ptr

        if isinstance(sites, str):
            sites = (sites,)
        ids = [self.site_id(s) for s in sites]
        K, N = len(ids), self.num_worlds
        if not 1 <= K <= 4:
            raise ValueError(f"solve_ik takes 1 .. 4 sites, not {K}")
        if int(max_iters) < 0 or not float(damping) > 0.0 or not float(tol) >= 0.0 or not float(max_step) > 0.0:
            raise ValueError("solve_ik needs max_iters >= 0, damping > 0, tol >= 0 and max_step > 0")
        sel = self._ik_dofs(dofs)

        def checked(x, what, shape):      # host only: a float32 tensor or array of shape [N, *shape], or [*shape]: the same rows in every world
            if not torch.is_tensor(x):
                x = np.asarray(x)
            if str(x.dtype).split(".")[-1] != "float32" or tuple(x.shape) not in ((N,) + shape, shape):
                raise ValueError(f"{what} must be float32 of shape {(N,) + shape} or {shape}, not {x.dtype} {tuple(x.shape)}")
            return x

        tp = checked(target_pos, "target_pos", (K, 3))
        tq = None if target_quat is None else checked(target_quat, "target_quat", (K, 4))
        q0 = None if qpos0 is None else checked(qpos0, "qpos0", (self.nq,))
        if mask is not None and tuple(mask.shape if hasattr(mask, "shape") else np.asarray(mask).shape) != (N,):
            raise ValueError(f"mask must have shape ({N},)")
        if out is not None:
            for x, shape, dt in zip(out, ((N, self.nq), (N,), (N,)), (torch.float32, torch.float32, torch.int32)):
                if not torch.is_tensor(x) or tuple(x.shape) != shape or x.dtype != dt or not x.is_cuda or not x.is_contiguous():
                    raise ValueError(f"out= takes contiguous device tensors: qpos float32 {(N, self.nq)}, err float32 {(N,)}, iters int32 {(N,)}")
        t = self._ensure()      # from here on the device
        if self._entry is None:
            raise RuntimeError("this BatchedSim is closed: its model handles are gone")
        rows = lambda x, shape: None if x is None else torch.as_tensor(x, device=self.device).expand((N,) + shape).contiguous()
        tp, tq, q0, m = rows(tp, (K, 3)), rows(tq, (K, 4)), rows(q0, (self.nq,)), self._mask(mask)
        if q0 is None:
            q0 = t["qpos"]
        qpos, err, iters = out if out is not None else (torch.empty((N, self.nq), dtype=torch.float32, device=self.device), torch.empty(N, dtype=torch.float32, device=self.device),
                                                        torch.empty(N, dtype=torch.int32, device=self.device))
        host = (ctypes.c_int * K)(*ids)
        ptr = lambda x: None if x is None or not x.numel() else x.data_ptr()
        b = _native.SimIkStruct(qpos0=q0.data_ptr(), mocap_pos=ptr(t["mocap_pos"]), mocap_quat=ptr(t["mocap_quat"]), target_pos=tp.data_ptr(), target_quat=ptr(tq), mask=ptr(m),
                                qpos=qpos.data_ptr(), err=err.data_ptr(), iters=iters.data_ptr(), site=ctypes.cast(host, ctypes.c_void_p),
                                dof_mask=None if sel is None else sel.ctypes.data, n_sites=K, max_iters=int(max_iters), clamp_limits=int(bool(clamp_limits)),
                                damping=float(damping), max_step=float(max_step), tol=float(tol), rot_weight=float(rot_weight))
        with torch.cuda.device(self.device):
            _native.check(self._L.grx_sim_ik(self._h, ctypes.byref(b), N, stream_ptr(self.device)))
        return qpos, err, iters

    # ------------------------------------------------------------------ status words (include/grx_capi.h grx_status_bits), as the env classes report them
    @property
    def status(self):
        """int16 view [N]: the GRX_STATUS_* flags of the last launch (0 = healthy)"""
        import torch

        return self._ensure()["status_words"].view(torch.int16).view(-1, 2)[:, 0]

    @property
    def status_sticky(self):
        """int16 view [N]: the same flags OR-accumulated over every launch since clear_status()"""
        import torch

        return self._ensure()["status_words"].view(torch.int16).view(-1, 2)[:, 1]

    def status_counts(self):
        from .core import status_counts

        return status_counts(self._ensure()["status_words"], self.num_worlds)

    def clear_status(self):
        self._ensure()["status_words"].zero_()

    # ------------------------------------------------------------------ checkpoints
    def get_state(self):
        """the state rows and the status words as host arrays (synchronises); the outputs are not state: forward() rebuilds them"""
        import torch

        t = self._ensure()
        torch.cuda.synchronize(self.device)
        d = {k: t[k].cpu().numpy().copy() for k in STATE + ("status_words",)}
        if self.param_names:      # the rows as written (a row a commit refused included: set_state commits them again, with the same outcome)
            d["params"] = {k: getattr(self._params, k).cpu().numpy().copy() for k in self.param_names}
        for k in self.applied:      # the named input rows under their names (xipos is an output)
            if k in APPLIED_INPUTS:
                d[k] = t[k].cpu().numpy().copy()
        return d

    def set_state(self, d):
        import torch

        t = self._ensure()
        for k in STATE:
            if k not in d:
                raise ValueError(f"state lacks {k!r}")
            if tuple(np.shape(d[k])) != tuple(t[k].shape):
                raise ValueError(f"state row {k!r} has shape {tuple(np.shape(d[k]))}, this simulation holds {tuple(t[k].shape)}")
        for k in STATE + (("status_words",) if "status_words" in d else ()):
            t[k].copy_(torch.from_numpy(np.ascontiguousarray(d[k], dtype=np.int32 if k == "status_words" else np.float32)).to(self.device))
        if "params" in d and self.param_names:      # (a state without the key leaves the parameters alone)
            rows = d["params"]
            if set(rows) != set(self.param_names):
                raise ValueError(f"state holds the parameters {sorted(rows)}, this simulation {sorted(self.param_names)}")
            for k in self.param_names:
                dst = getattr(self._params, k)
                if tuple(np.shape(rows[k])) != tuple(dst.shape):
                    raise ValueError(f"parameter row {k!r} has shape {tuple(np.shape(rows[k]))}, this simulation holds {tuple(dst.shape)}")
                dst.copy_(torch.from_numpy(np.ascontiguousarray(rows[k], dtype=np.float32)).to(self.device))
            self.commit_params()
        elif "params" in d:
            raise ValueError("the state carries model parameters and this simulation names none")
        for k in APPLIED_INPUTS:      # the rule of "params": a state without the key leaves the row alone
            if k not in d:
                continue
            if k not in self.applied:
                raise ValueError(f"the state carries {k!r} and this simulation does not name it (BatchedSim(..., applied=...))")
            if tuple(np.shape(d[k])) != tuple(t[k].shape):
                raise ValueError(f"state row {k!r} has shape {tuple(np.shape(d[k]))}, this simulation holds {tuple(t[k].shape)}")
            t[k].copy_(torch.from_numpy(np.ascontiguousarray(d[k], dtype=np.float32)).to(self.device))

    def close(self):
        from .core import release_models

        if self._t is not None:
            import torch

            torch.cuda.synchronize(self.device)
        if self.__dict__.get("_p") is not None:
            self._params = None
            self._L.grx_sim_params_destroy(self._p)
            self._p = None
        if self.__dict__.get("_tri") is not None:
            self._L.grx_sim_trimesh_destroy(self._tri)
            self._tri = None
        self._entry = None      # (it holds the parameter object's pointer: no launch after close)
        release_models(self, ("_h", "_h_big"))
        self.lane = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
