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
accelerometer = R'(c - g), frameangacc = alpha.  ``- g`` is MuJoCo's convention that the world body accelerates with ``-gravity`` (an accelerometer at rest reads +9.81 along world
z); it is the DEFINITION of ``framelinacc`` here as well.  A world that names ``gravity`` among ``model_params`` reads its own committed row.  A positive ``cutoff`` clamps a reading to
[-cutoff, cutoff] (not the quaternion and axis types); ``noise`` is ignored.  Refused by name, with the reason: ``touch`` (``outputs=("sensordata",)`` with ``touch_filter``),
``rangefinder`` (``sim.rangefinder()``), ``force`` / ``torque`` (they need cfrc_int / cfrc_ext, which the engine does not form), frame sensors on a ``body`` (the inertial frame),
``geom`` or ``camera``, any ``reftype``, every other type, and an ``xbody`` the compiler merged into its parent or a site ``keep_sites`` dropped.
WHICH PASS: all readings belong to ONE forward pass, with that pass's own qvel and qacc.  After ``forward()``: that pass.  After ``step(n)`` of an Euler model: the last substep's pass,
before its integration.  Of an RK4 model: the FIRST stage's pass of the last substep -- ``mj_step`` runs ``mj_forward`` with sensors, then ``mj_RungeKutta`` with the sensors skipped --
which differs on purpose from the fourth-stage pass of the other outputs.  Either way the readings after ``step(n)`` are those of ``forward()`` at the state ``step(n - 1)`` left.
Sensors are not state: ``reset()``'s ``forward()`` refreshes them, ``get_state`` / ``set_state`` do not carry them.  Naming one routes the launch through grx_sim_step_sns.

    sim = grx.BatchedSim("quadruped.xml", 4096, sensors=("imu_acc", "imu_gyro", "imu_quat", "hip_pos", "hip_vel"))
    sim.step(nstep=5)
    obs = torch.cat([sim.sensor_data, sim.ctrl], dim=1)                                            # or sim.sensor("imu_acc"): [N, 3]

RAYS (``mj_ray``, rangefinders, lidar): ``sim.ray(origin, direction)`` casts R rays per world -- ``origin`` / ``direction`` [N, R, 3] (or [R, 3]) in world coordinates, ``direction``
of any length -- and returns ``(dist [N, R] float32, geom [N, R] int32)``: the ray parameter of the nearest hit (metres for a unit direction) and the geom hit, -1.0 / -1 for none.
``sim.ray_sites(sites, local_dir)`` starts the rays at sites and skips each site's own body; ``sim.rangefinder()`` is [N, n_rangefinder], one reading per ``<rangefinder>`` of the MJCF
(along the site's +z, -1 for none or beyond the sensor's cutoff).  The rays see the body poses of the LAST launch -- ``outputs`` must name ``xpos`` and ``xquat`` (and ``site_xpos`` /
``site_xmat`` for the site variants) -- so exactly what ``MjData.geom_xpos`` holds then: exact after ``forward()``, one substep stale after ``step()``.  Three deviations from ``mj_ray``:
the rays see the COMPILED model's geoms, i.e. the collidable ones (visual geoms do not exist there); a mesh geom is its CONVEX HULL, the shape the engine collides with; there are no
geom groups.  A mesh geom whose only candidate pairs are with planes (or that has none) keeps no full hull in the compiled model: the ray calls raise a ``ValueError`` that names
it rather than cast through it.  The calls run a kernel of their own (grx_sim_ray / grx_sim_ray_sites) on torch's current stream and never synchronise; rays are not state.

    sim = grx.BatchedSim("maze_agent.xml", 4096, outputs=("xpos", "xquat", "site_xpos", "site_xmat"))
    fan = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros_like(ang)], dim=1)             # [64, 3] in the frame of the site "lidar"
    sim.step(nstep=5)
    dist, geom = sim.ray_sites("lidar", fan, max_dist=10.0)                                        # [N, 64]

Not here: shape-specialised kernels for user models, split or cost-ordered launches, a handle in libgrx_env.so, keyframes, per-world geometry or poses,
force / torque sensors (cfrc_int, cfrc_ext), sensor reference frames and noise, MuJoCo's contact order, elliptic cones, rays against visual geoms or mesh triangles, geom groups, height fields, cameras.
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
_SIM_BLOCKS = ("_dyn", "_con", "_frc", "_sns")
_SIM_ENTRIES = (("_sns", "grx_sim_step_sns", True, 4), ("_frc", "grx_sim_step_frc", True, 3), ("_con", "grx_sim_step_con", True, 2), ("_p", "grx_sim_step_params", True, 1),
                ("_dyn", "grx_sim_step_dyn", False, 1), (None, "grx_sim_step", False, 0))
APPLIED = ("qfrc_applied", "xfrc_applied", "xipos")      # grx_sim_applied, in its order: two inputs the caller writes, one output
APPLIED_INPUTS = ("qfrc_applied", "xfrc_applied")
# grx_sim_sensors: the type and object numbers of csrc/grx_sim_sensors.h, in its order
SENSOR_TYPES = ("jointpos", "jointvel", "actuatorpos", "actuatorvel", "actuatorfrc", "jointactuatorfrc", "framepos", "framequat", "framexaxis", "frameyaxis", "framezaxis",
                "framelinvel", "frameangvel", "velocimeter", "gyro", "framelinacc", "frameangacc", "accelerometer")
SENSOR_OBJECTS = ("joint", "actuator", "site", "xbody")
_SENSOR_JOINT, _SENSOR_ACTUATOR, _SENSOR_SITE_ONLY = ("jointpos", "jointvel", "jointactuatorfrc"), ("actuatorpos", "actuatorvel", "actuatorfrc"), ("velocimeter", "gyro", "accelerometer")
_SENSOR_NO_CUTOFF = ("framequat", "framexaxis", "frameyaxis", "framezaxis")
MAXJAC = 16      # GRX_SIM_MAXJAC: the site selection rides inside the launch's argument block


def _table_maxcon(req):
    """the contact-list capacity of a handle whose model requests `req` (csrc/grx_host_model.h: the request if it lies in 1 .. 64, else the default 32)"""
    return req if 0 < req <= 64 else 32


class _Params:
    """sim.params: one attribute per named table, the [N, ...] device tensor the caller writes"""

    def __repr__(self):
        return "params(" + ", ".join(f"{k}{tuple(v.shape)}" for k, v in self.__dict__.items()) + ")"


class BatchedSim:
    def __init__(self, model, num_worlds, device="cuda:0", capacity=None, overflow="rerun", outputs=(), compile_kwargs=None, jac_sites=None, model_params=(), contacts=(), applied=(), sensors=()):
        """model: path of an MJCF file, or a mjcf.CompiledModel.  capacity: dict(maxcon=, maxefc=, jpool=) of the tables the step launch runs on (None: the compiler's
        default, 32 contacts / 144 rows / 2 032 Jacobian words).  overflow: "rerun" -- a world that exceeds a table in some substep is left untouched by the step launch and run
        again, right behind it, on the large tables (core.RERUN_CAPACITY), so no contact is dropped; "flag" -- it goes on with the excess contacts dropped and the status bits
        CON_OVERFLOW / EFC_OVERFLOW say so.  outputs: the MjData fields to allocate and write, any of sim.OUTPUTS.  compile_kwargs: passed to compile_mjcf (touch_filter,
        keep_sites, mutate, ...).  jac_sites: the names of the sites whose Jacobians site_jacp / site_jacr hold, in the order of their rows (None: every site of the model, which must
        then have at most 16).  model_params: the tables that are per world, any of sim.PARAMS (module docstring).  contacts: the members of the contact list to allocate and write, any of sim.CONTACTS
        (module docstring).  applied: the applied-force inputs and xipos, any of sim.APPLIED (module docstring).  sensors: names of <sensor> children of the MJCF, or "all" (module docstring, SENSORS).  Nothing is allocated and no library is loaded before the first tensor is touched or the first launch: the name lookups work without a device."""
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
        self._h = self._h_big = self.lane = self._p = self._frc = self._sns = None

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
        if kind in ("force", "torque"):
            raise ValueError(f"{who}: force and torque sensors need cfrc_int / cfrc_ext, which the engine does not form")
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
                    qfrc_applied=(n, self.nv), xfrc_applied=(n, self.nbody, 6), xipos=(n, self.nbody, 3))

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
        for k in STATE + self.outputs + self.contacts + self.applied:
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
        if name in STATE or name == "status_words" or name in self.__dict__.get("outputs", ()) or name in self.__dict__.get("contacts", ()) or name in self.__dict__.get("applied", ()):
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
    def _ray_need(self, what, needed):
        missing = [o for o in needed if o not in self.outputs]
        if missing:
            raise ValueError(f"{what} casts against the body poses of the last launch and needs the output(s) {missing}: BatchedSim(..., outputs={self.outputs + tuple(missing)})")
        tb = self.model.tables
        kind, hull = np.asarray(tb["geom_type"]).reshape(-1), np.asarray(tb["geom_hullnum"]).reshape(-1)
        bare = [int(g) for g in np.nonzero(kind == 7)[0] if g >= len(hull) or hull[g] < 4]
        if bare:      # the compiler keeps a mesh's full hull only for hull-vs-convex candidate pairs: a ray would pass through such a geom unseen
            by_id = {i: name for name, i in self.model.names.get("geom", {}).items()}
            raise ValueError(f"{what}: mesh geom(s) {[by_id.get(g, g) for g in bare]} have no full hull in the compiled model (a mesh keeps it only when it has a candidate pair with a "
                             "sphere, capsule, ellipsoid, cylinder, box or mesh geom; these meet planes only, or nothing), so rays cannot see them")

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

    def _ray_launch(self, fn, block, n_rays, keep):
        import torch

        from . import _native
        from .core import stream_ptr

        self._ray_keep = keep      # the inputs stay alive until the next ray call has replaced them (the launch is only enqueued)
        with torch.cuda.device(self.device):
            _native.check(fn(self._h, ctypes.byref(block), self.num_worlds, int(n_rays), stream_ptr(self.device)))

    def ray(self, origin, direction, exclude_body=None, max_dist=0.0, include_static=True, mask=None, out=None):
        """mj_ray for R rays in every world: origin, direction [N, R, 3] device tensors in world coordinates ([R, 3]: the same rays in every world); direction need not be unit.
        Returns (dist [N, R] float32, geom [N, R] int32): the parameter t of the nearest hit (metres for a unit direction) and the id of the geom hit (sim.geom_id), or -1.0 / -1
        for no hit, a hit beyond max_dist (when positive), a zero or non-finite direction.  exclude_body: a body name or compiled body id, or a list / tensor of R of them (-1:
        none): that body's geoms are skipped (mj_ray's bodyexclude).  include_static=False skips the geoms of the world body.  mask: only the worlds with a non-zero entry are
        written; the rows of the others read -1.0 / -1 in fresh tensors and keep their bits in out= tensors.  out=(dist, geom): write into these tensors.  Casts against the xpos / xquat of the LAST launch (exact after forward(), one substep stale after step()).
        Enqueues on torch's current stream; never synchronises."""
        import torch

        from . import _native

        self._ray_need("ray()", ("xpos", "xquat"))
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
        self._ray_launch(self._L.grx_sim_ray, b, n_rays, (o, d, e, m))
        return dist, geom

    def ray_sites(self, sites, local_dir, exclude_own_body=True, exclude_body=None, max_dist=0.0, include_static=True, mask=None, out=None):
        """R rays that start at sites: ray r starts at site sites[r] (a name or id; one name: every ray) and runs along local_dir[r] ([R, 3], in the site's frame), in every
        world.  exclude_own_body: the geoms of the site's body are skipped (the rangefinder rule); the other arguments and the result are those of ray().  Reads site_xpos /
        site_xmat of the last launch as well.  The first call with a list of sites the model handle has not seen uploads it (one blocking copy; the handle keeps the 64 most recent
        lists); every later call with that list only enqueues."""
        import torch

        from . import _native

        self._ray_need("ray_sites()", ("xpos", "xquat", "site_xpos", "site_xmat"))
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
        self._ray_launch(self._L.grx_sim_ray_sites, b, n_rays, (l, e, m, host))
        return dist, geom

    @property
    def n_rangefinder(self):
        return len(self.model.info.get("rangefinder", ()))

    def rangefinder_id(self, name):
        """column of the <rangefinder> sensor `name` in rangefinder()"""
        return self._lookup("rangefinder", name)

    def rangefinder(self, mask=None):
        """[N, n_rangefinder] float32: the reading of every <rangefinder> sensor of the MJCF, in sensor order -- the distance along the +z axis of the sensor's site to the
        nearest geom that does not belong to the site's body, -1 for none or for one beyond the sensor's positive cutoff (mjSENS_RANGEFINDER, over the geoms ray() sees).
        mask: the rows of the worlds it leaves out read -1."""
        import torch

        rows = self.model.info.get("rangefinder", ())
        if not rows:
            raise ValueError("the model has no <rangefinder> sensor")
        lost = [name for name, k in self.model.names["rangefinder"].items() if rows[k]["site"] not in self.model.names["site"]]
        if lost:
            raise ValueError(f"the site of rangefinder(s) {sorted(lost)} is not among the model's sites (the sensor names none, or keep_sites dropped it: compile_kwargs=dict(keep_sites=...))")
        self._ray_need("rangefinder()", ("xpos", "xquat", "site_xpos", "site_xmat"))
        self._ensure()
        if self.__dict__.get("_rf") is None:
            self._rf = (torch.tensor([[0.0, 0.0, 1.0]] * len(rows), device=self.device), torch.tensor([[max(float(r["cutoff"]), 0.0) for r in rows]], dtype=torch.float32, device=self.device))
        z, cut = self._rf
        dist, _ = self.ray_sites([r["site"] for r in rows], z, exclude_own_body=True, mask=mask)
        beyond = (cut > 0) & (dist > cut)      # each sensor's own cutoff
        if mask is not None:
            beyond &= self._mask(mask).bool()[:, None]
        return dist.masked_fill_(beyond, -1.0)

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
        self._entry = None      # (it holds the parameter object's pointer: no launch after close)
        release_models(self, ("_h", "_h_big"))
        self.lane = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
