"""Touch sensors zone by zone (tests/test_cpu_touch.py on the emulator and the oracle, tests/test_gpu_touch.py on the device): generated MJCF scenes, their start states,
the oracle reader and the comparisons both files share.  Plain Python and numpy; the reference is tests/touch_refs.py.

Every scene is a few free bodies pressed 0.3 .. 3 mm into a plane or into each other; one world per start, fp32-valued starts, Euler unless said otherwise.  A scene is
built from its zone table: each zone is written down here with its pose IN THE FRAME OF THE BODY THAT SURVIVES COMPILATION (a site on a static child body is written into
the MJCF in the child's frame, by the inverse of the child's pose), so the compiler's touch_* tables are checked against the intent and not against themselves.

types ...... one free ball on the plane: one contact, whose ray runs straight down from the contact point whatever the ball's orientation.  Sphere, box and cylinder zones,
             each in four placements about that contact -- `in` (the contact inside the zone), `hit` (the zone 2 cm down the ray), `away` (2 cm up the ray: a miss that a
             wrong sign turns into a hit) and `beside` (2.5 cm off the ray's line: a miss either way) -- each with its own offset and rotation on the tilted ball; and a
             second copy of all twelve on a static child body the compiler merges into the ball.
rows1/4/6 .. the same scene at condim 1, 4 and 6 (types is condim 3): the normal force is the sum of 1, 4, 6 and 10 rows.
gap ........ the same ball with margin 0.004 and gap 0.001, held 3.5 mm above the plane: a contact without constraint rows, every reading exactly 0; a second ball is pressed
             in, so the world does have rows.
rk4 ........ types with integrator="RK4", for the self-consistency check alone.
order-ab ... a ball A resting obliquely on a ball B that rests on the plane, zones on both; A comes first in the MJCF.
order-ba ... the same with B first: the A - B contact's geom1 / geom2 are swapped, so each zone's body is the contact's first body in one scene and its second in the other.
both ....... the same pair at another angle: one contact feeds a zone on each body, with opposite ray directions.
axes ....... a free box flat on the plane (world 0 with the identity orientation), axis-aligned zones at its four bottom corners: the ray is (0, 0, -1) in the zone frame, so
             two of the box routine's three axes are skipped and a standing cylinder takes its caps-only path; a cylinder lying on its side takes the side-only path, once hit,
             once missed past its cap, once missed beside.
many ....... a tilted box on the plane (four contacts with four different forces): a pad over two corners, a pad over all four, a sphere at one, a long cylinder under one
             diagonal, a pad on the top face -- overlapping zones on one body; five small balls on vertical slides, each with a zone, down in worlds 1 and 3 and up in the air
             otherwise (a body without any contact).  With an 8-contact list worlds 1 and 3 (nine contacts) take the re-run path.
grid70 ..... a tilted box on the plane with a 7 x 10 grid of zones on its bottom face (ntouch = 70 > 64 lanes): the zones at the corners contain the contacts; the rows next to the
             y edges hang 12 mm lower and reach under the corners, so the corner rays hit them from outside."""
import os

import numpy as np

import engine_matrix_cases as C
import sim_cases as S
import sim_contact_cases as K
import touch_refs as R

N = S.N_WORLDS
MIN_MARGIN = 1e-3      # metres: every (zone, contact) decision of every world
MIN_FORCE = 0.05       # newtons: every counted normal force
EPS32 = float(np.finfo(np.float32).eps)
CON_OUTPUTS = ("sensordata", "ncon", "nefc", "xpos", "xquat")
PLACEMENTS = ("in", "hit", "away", "beside")
_TYPE = {"sphere": R.SPHERE, "box": R.BOX, "cylinder": R.CYLINDER}
_SIZES = {"sphere": (0.009, 0.0, 0.0), "box": (0.012, 0.009, 0.007), "cylinder": (0.009, 0.007, 0.0)}
_OFFSET = {"in": (0.002, -0.0015, 0.001), "hit": (0.002, 0.001, -0.020), "away": (0.002, 0.001, 0.020), "beside": (0.025, 0.003, -0.010)}      # about the contact, world axes
_HALF = np.sqrt(0.5)


def _s(v):
    return " ".join(repr(float(x)) for x in np.atleast_1d(v))


def _qinv(q):
    return np.r_[q[0], -np.asarray(q[1:])]


def zone(name, body, kind, pos, quat, size, child=None, tag=None):
    return dict(name=name, body=body, type=_TYPE[kind], pos=np.asarray(pos, dtype=np.float64), quat=np.asarray(quat, dtype=np.float64) / np.linalg.norm(quat),
                size=np.asarray(size, dtype=np.float64), child=child, tag=tag)


def _site(z, child_pose=None):
    """the <site> of a zone, in the frame it is written in: the surviving body's, or the static child's (child_pose = its pos, quat on that body)"""
    pos, quat = z["pos"], z["quat"]
    if child_pose is not None:
        pc, qc = child_pose
        pos, quat = C.quat_rot(_qinv(qc), pos - pc), C.quat_mul(_qinv(qc), quat)
    kind = {R.SPHERE: "sphere", R.BOX: "box", R.CYLINDER: "cylinder"}[z["type"]]
    n = {R.SPHERE: 1, R.BOX: 3, R.CYLINDER: 2}[z["type"]]
    return f'<site name="{z["name"]}" type="{kind}" size="{_s(z["size"][:n])}" pos="{_s(pos)}" quat="{_s(quat)}"/>'


def _sensors(zones):
    return "<sensor>" + "".join(f'<touch name="t_{z["name"]}" site="{z["name"]}"/>' for z in zones) + "</sensor>"


def _head(rk4=False):
    return f'<mujoco><compiler angle="radian"/><option timestep="0.002"{" integrator=" + chr(34) + "RK4" + chr(34) if rk4 else ""}/>'


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the ball scenes
_BALL_R = 0.05
_BALL_Q0 = C.axis_angle([1.0, 2.0, 3.0], 0.7)      # the ball's nominal orientation: nothing is axis-aligned
_CHILD = (np.array([0.004, -0.003, 0.002]), C.axis_angle([0.3, -1.0, 0.5], 0.9))      # the static child's pose on the ball


def _ball_zones(depth_nom):
    """24 zones about the ball's plane contact at the nominal pose: 3 types x 4 placements on the ball, and again on its static child"""
    rng = np.random.default_rng([0x7B1, 24])
    contact = np.array([0.0, 0.0, -(_BALL_R - depth_nom / 2.0)])      # from the ball's centre, world axes
    out = []
    for where in ("", "c"):
        for kind in ("sphere", "box", "cylinder"):
            for pl in PLACEMENTS:
                centre = contact + np.array(_OFFSET[pl]) + rng.uniform(-8e-4, 8e-4, 3)
                q_world = C._unit(rng, 4)
                out.append(zone(f"{where}{kind[:3]}_{pl}", "ball", kind, C.quat_rot(_qinv(_BALL_Q0), centre), C.quat_mul(_qinv(_BALL_Q0), q_world), _SIZES[kind],
                                child="plate" if where else None, tag=(kind, pl)))
    return out


def _ball_scene(condim=3, rk4=False, gap=False):
    depth_nom = -3.5e-3 if gap else 1.65e-3
    zones = _ball_zones(depth_nom)
    extra = ' margin="0.004" gap="0.001"' if gap else ""
    own = "".join(_site(z) for z in zones if z["child"] is None)
    kid = "".join(_site(z, _CHILD) for z in zones if z["child"] is not None)
    press = ""
    if gap:      # a second ball that is pressed in: the world has rows, and one reading is not zero
        zones.append(zone("press_in", "press", "sphere", [0.001, -0.001, -0.029], [1, 0, 0, 0], (0.008, 0, 0)))
        press = f'<body name="press" pos="0.3 0 0.03"><freejoint name="pressj"/><geom name="pressg" type="sphere" size="0.03" mass="0.1" condim="3"/>{_site(zones[-1])}</body>'
    xml = (f'{_head(rk4)}<worldbody><geom name="floor" type="plane" size="2 2 0.1" condim="{condim}"{extra}/>'
           f'<body name="ball" pos="0 0 {_BALL_R}"><freejoint name="ballj"/><geom name="ballg" type="sphere" size="{_BALL_R}" mass="0.2" condim="{condim}" friction="0.8 0.02 0.001"{extra}/>{own}'
           f'<body name="plate" pos="{_s(_CHILD[0])}" quat="{_s(_CHILD[1])}"><geom type="box" size="0.01 0.01 0.002" mass="0.01" contype="0" conaffinity="0"/>{kid}</body></body>'
           f'{press}</worldbody>{_sensors(zones)}</mujoco>')
    return xml, zones


def _free(model, q, v, joint, pos, quat, vel=None):
    a, d = _adr(model, joint)
    q[a:a + 3], q[a + 3:a + 7] = pos, quat
    if vel is not None:
        v[d:d + 6] = vel


def _adr(model, joint):
    j = model.names["joint"][joint]
    return int(np.asarray(model.tables["jnt_qposadr"]).reshape(-1)[j]), int(np.asarray(model.tables["jnt_dofadr"]).reshape(-1)[j])


def _empty(model, n):
    nq, nv, nu, nm = S._dims(model)
    return np.zeros((n, nq)), np.zeros((n, nv)), dict(ctrl=np.zeros((n, nu)), mocap_pos=np.zeros((n, nm, 3)), mocap_quat=np.zeros((n, nm, 4)))


def _ball_states(gap):
    def states(model, n, seed):
        q, v, rest = _empty(model, n)
        for i in range(n):
            r = S._world_rng(seed, i)
            if gap:
                _free(model, q[i], v[i], "ballj", [0.02, -0.01, _BALL_R + 3.5e-3], _BALL_Q0)
                _free(model, q[i], v[i], "pressj", [0.3, 0.0, 0.03 - 1.5e-3], [1, 0, 0, 0])
                continue
            quat = C.quat_mul(C.axis_angle(C._unit(r, 3), 0.03 * r.standard_normal()), _BALL_Q0)
            _free(model, q[i], v[i], "ballj", np.r_[0.05 * r.standard_normal(2), _BALL_R - r.uniform(3e-4, 3e-3)], quat,
                  np.r_[0.05 * r.standard_normal(2), 0.0, 0.2 * r.standard_normal(3)])
        return dict(qpos=q, qvel=v, **rest)
    return states


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the two-ball scenes
_RA, _RB = 0.03, 0.04
_QA0, _QB0 = C.axis_angle([2.0, -1.0, 1.0], 1.1), C.axis_angle([-1.0, 1.0, 2.0], 0.8)


def _pair_geometry(theta, phi, d_b=1.5e-3, d_ab=1.5e-3):
    """world positions at the nominal pose: B's centre, A's centre, the direction u from B to A, the A - B contact point, the B - plane contact point"""
    u = np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])
    cb = np.array([0.0, 0.0, _RB - d_b])
    ca = cb + (_RA + _RB - d_ab) * u
    return cb, ca, u, cb + (_RB - d_ab / 2.0) * u, np.array([0.0, 0.0, -d_b / 2.0])


def _pair_scene(first, theta, phi):
    cb, ca, u, pc, pf = _pair_geometry(theta, phi)
    rng = np.random.default_rng([0x7B2, int(1000 * theta)])
    side = np.cross(u, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)

    def on(body, name, kind, centre, tag):
        c0, q0 = (ca, _QA0) if body == "A" else (cb, _QB0)
        return zone(name, body, kind, C.quat_rot(_qinv(q0), centre + rng.uniform(-8e-4, 8e-4, 3) - c0), C.quat_mul(_qinv(q0), C._unit(rng, 4)), _SIZES[kind], tag=tag)

    # A's zones see the ray run from the contact towards B (-u), B's towards A (+u); B's also see the plane contact, whose ray runs down
    zones = [on("A", "a_in", "sphere", pc, "in"), on("A", "a_hit", "box", pc - 0.018 * u, "hit"), on("A", "a_away", "cylinder", pc + 0.018 * u, "away"),
             on("A", "a_beside", "box", pc - 0.010 * u + 0.027 * side, "beside"),
             on("B", "b_in", "box", pc, "in"), on("B", "b_hit", "cylinder", pc + 0.018 * u, "hit"), on("B", "b_away", "sphere", pc - 0.018 * u, "away"),
             on("B", "b_beside", "cylinder", pc + 0.010 * u - 0.027 * side, "beside"),
             on("B", "b_floor", "cylinder", pf, "in"), on("B", "b_under", "sphere", pf - [0.0, 0.0, 0.018], "hit")]
    body = {
        "A": f'<body name="A" pos="{_s(ca)}" quat="{_s(_QA0)}"><freejoint name="Aj"/><geom name="Ag" type="sphere" size="{_RA}" mass="0.2" condim="3"/>' + "".join(_site(z) for z in zones if z["body"] == "A") + "</body>",
        "B": f'<body name="B" pos="{_s(cb)}" quat="{_s(_QB0)}"><freejoint name="Bj"/><geom name="Bg" type="sphere" size="{_RB}" mass="0.3" condim="3"/>' + "".join(_site(z) for z in zones if z["body"] == "B") + "</body>"}
    order = ("A", "B") if first == "A" else ("B", "A")
    xml = f'{_head()}<worldbody><geom name="floor" type="plane" size="2 2 0.1" condim="3"/>{body[order[0]]}{body[order[1]]}</worldbody>{_sensors(zones)}</mujoco>'
    return xml, zones


def _pair_states(theta, phi):
    def states(model, n, seed):
        q, v, rest = _empty(model, n)
        for i in range(n):
            r = S._world_rng(seed, i)
            cb, ca, u, _, _ = _pair_geometry(theta, phi, d_b=r.uniform(3e-4, 3e-3), d_ab=r.uniform(3e-4, 3e-3))
            shift = np.r_[0.01 * r.standard_normal(2), 0.0]      # close to the origin: the ulp of a coordinate is what the one-ulp jitter moves a contact by
            for name, c0, q0 in (("Aj", ca, _QA0), ("Bj", cb, _QB0)):
                _free(model, q[i], v[i], name, c0 + shift, C.quat_mul(C.axis_angle(C._unit(r, 3), 0.03 * r.standard_normal()), q0),
                      np.r_[0.02 * r.standard_normal(3), 0.2 * r.standard_normal(3)])
        return dict(qpos=q, qvel=v, **rest)
    return states


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the box scenes
_BX = 0.05      # half size of the box in x and y
_LIE = (_HALF, 0.0, _HALF, 0.0)      # a cylinder zone on its side: its axis along the body's x


def _box_body(hz, zones, mass=0.3):
    return (f'<body name="box" pos="0 0 {hz}"><freejoint name="boxj"/><geom name="boxg" type="box" size="{_BX} {_BX} {hz}" mass="{mass}" condim="3"/>'
            + "".join(_site(z) for z in zones if z["body"] == "box") + "</body>")


def _axes_scene():
    h, e = _BX, [1, 0, 0, 0]
    cyl, lie, box, sph = (0.01, 0.008, 0), (0.008, 0.012, 0), (0.01, 0.008, 0.006), (0.009, 0, 0)
    zones = [zone("cyl_stand_in", "box", "cylinder", [h, h, -h], e, cyl, tag="in"), zone("cyl_stand_hit", "box", "cylinder", [h + 0.002, h - 0.001, -h - 0.025], e, cyl, tag="hit"),
             zone("cyl_stand_away", "box", "cylinder", [h + 0.001, h, -h + 0.025], e, cyl, tag="away"), zone("cyl_stand_beside", "box", "cylinder", [h + 0.018, h, -h - 0.025], e, cyl, tag="beside"),
             zone("cyl_lie_hit", "box", "cylinder", [-h + 0.003, h, -h - 0.02], _LIE, lie, tag="hit"), zone("cyl_lie_past_cap", "box", "cylinder", [-h + 0.02, h, -h - 0.02], _LIE, lie, tag="beside"),
             zone("cyl_lie_beside", "box", "cylinder", [-h, h - 0.02, -h - 0.02], _LIE, lie, tag="beside"), zone("cyl_lie_away", "box", "cylinder", [-h, h, -h + 0.02], _LIE, lie, tag="away"),
             zone("box_in", "box", "box", [-h, -h, -h], e, box, tag="in"), zone("box_hit", "box", "box", [-h - 0.002, -h + 0.001, -h - 0.02], e, box, tag="hit"),
             zone("box_away", "box", "box", [-h, -h, -h + 0.02], e, box, tag="away"), zone("box_beside", "box", "box", [-h - 0.02, -h, -h - 0.02], e, box, tag="beside"),
             zone("sph_in", "box", "sphere", [h, -h, -h], e, sph, tag="in"), zone("sph_hit", "box", "sphere", [h + 0.001, -h - 0.002, -h - 0.02], e, sph, tag="hit"),
             zone("sph_away", "box", "sphere", [h, -h, -h + 0.02], e, sph, tag="away"), zone("sph_beside", "box", "sphere", [h + 0.018, -h, -h - 0.02], e, sph, tag="beside")]
    return f'{_head()}<worldbody><geom name="floor" type="plane" size="2 2 0.1" condim="3"/>{_box_body(_BX, zones)}</worldbody>{_sensors(zones)}</mujoco>', zones


MANY_BALLS = 5
MANY_DOWN = (1, 3)      # the worlds in which the small balls are down
MANY_CAPACITY = dict(maxcon=8, maxefc=48, jpool=256)      # the fast tables of the re-run test: 4 box contacts fit, 4 + 5 do not


def _many_scene():
    h = _BX
    zones = [zone("pad2", "box", "box", [0, h, -h], C.axis_angle([0, 0, 1], 0.1), (0.06, 0.012, 0.006)), zone("pad4", "box", "box", [0, 0, -h], [1, 0, 0, 0], (0.06, 0.06, 0.005)),
             zone("pad1", "box", "sphere", [h, h, -h], [1, 0, 0, 0], (0.012, 0, 0)),
             zone("pad_diag", "box", "cylinder", [0, 0, -h], C.quat_mul(C.axis_angle([0, 0, 1], np.pi / 4), np.array(_LIE)), (0.01, 0.08, 0)),
             zone("pad_top", "box", "box", [0, 0, h], [1, 0, 0, 0], (0.06, 0.06, 0.005))]
    balls = ""
    for k in range(MANY_BALLS):
        z = zone(f"ball{k}_zone", f"s{k}", "sphere", [0.001, 0.0, -0.019], [1, 0, 0, 0], (0.008, 0, 0))
        zones.append(z)
        balls += (f'<body name="s{k}" pos="{0.2 + 0.06 * k:.2f} 0.2 0.02"><joint name="z{k}" type="slide" axis="0 0 1" damping="0.2"/>'
                  f'<geom type="sphere" size="0.02" mass="{0.05 + 0.01 * k:.2f}" condim="3"/>{_site(z)}</body>')
    return f'{_head()}<worldbody><geom name="floor" type="plane" size="2 2 0.1" condim="3"/>{_box_body(_BX, zones)}{balls}</worldbody>{_sensors(zones)}</mujoco>', zones


GRID = (7, 10)
_GRID_HZ = 0.02


def _grid_scene():
    zones = []
    for i in range(GRID[0]):
        for j in range(GRID[1]):
            x, y = -_BX + i * 2 * _BX / (GRID[0] - 1), -_BX + j * 2 * _BX / (GRID[1] - 1)
            low = j in (1, GRID[1] - 2)
            zones.append(zone(f"g{i}_{j}", "box", "box", [x, y, -_GRID_HZ - (0.012 if low else 0.0)], [1, 0, 0, 0], (0.006, 0.014 if low else 0.0045, 0.004)))
    return f'{_head()}<worldbody><geom name="floor" type="plane" size="2 2 0.1" condim="3"/>{_box_body(_GRID_HZ, zones)}</worldbody>{_sensors(zones)}</mujoco>', zones


def _box_states(hz, tilt, balls=0):
    def states(model, n, seed):
        q, v, rest = _empty(model, n)
        for i in range(n):
            r = S._world_rng(seed, i)
            yaw = 0.0 if (i == 0 and tilt == 0.0) else r.uniform(-np.pi, np.pi)
            quat = C.quat_mul(C.axis_angle([0, 0, 1], yaw), C.axis_angle(np.r_[C._unit(r, 2), 0.0], tilt * r.uniform(0.5, 1.0))) if tilt else C.axis_angle([0, 0, 1], yaw)
            depth = r.uniform(1.2e-3, 2.2e-3) if tilt else r.uniform(3e-4, 3e-3)
            _free(model, q[i], v[i], "boxj", np.r_[0.05 * r.standard_normal(2), hz - depth], quat,
                  np.r_[0.05 * r.standard_normal(2), 0.0, 0.0, 0.0, 0.2 * r.standard_normal()] if tilt else None)      # the flat box stands still: a sliding one unloads a corner
            for k in range(balls):
                a, d = _adr(model, f"z{k}")
                q[i, a] = -r.uniform(5e-4, 2e-3) if i in MANY_DOWN else 0.1 + 0.02 * k      # the joint coordinate is the height above the resting pose
                v[i, d] = 0.05 * r.standard_normal()
        return dict(qpos=q, qvel=v, **rest)
    return states


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, built, states, seed, n=N, nsteps=(0, 1), consistency_only=False):
        self.name, (self.xml, self.zones), self.n, self.nsteps, self.consistency_only = name, built, n, nsteps, consistency_only
        S._STATES["touch-" + name] = states
        self.scene = S.Scene("touch-" + name, self.xml, seed, compile_kwargs=dict(touch_filter=lambda sensor: True))

    model = property(lambda self: self.scene.model)
    states = property(lambda self: self.scene.states(self.n))


CASES = {c.name: c for c in (
    Case("types", _ball_scene(), _ball_states(False), 31),
    Case("rows1", _ball_scene(condim=1), _ball_states(False), 32),
    Case("rows4", _ball_scene(condim=4), _ball_states(False), 33),
    Case("rows6", _ball_scene(condim=6), _ball_states(False), 34),
    Case("gap", _ball_scene(gap=True), _ball_states(True), 35, n=1),
    Case("rk4", _ball_scene(rk4=True), _ball_states(False), 36, nsteps=(1,), consistency_only=True),
    Case("order-ab", _pair_scene("A", 0.3, 0.7), _pair_states(0.3, 0.7), 37),
    Case("order-ba", _pair_scene("B", 0.3, 0.7), _pair_states(0.3, 0.7), 37),
    Case("both", _pair_scene("A", 0.6, -2.0), _pair_states(0.6, -2.0), 38),
    Case("axes", _axes_scene(), _box_states(_BX, 0.0), 39),
    Case("many", _many_scene(), _box_states(_BX, 0.006, MANY_BALLS), 40),
    Case("grid70", _grid_scene(), _box_states(_GRID_HZ, 0.006), 41),
)}
COMPARED = [c for c in CASES if not CASES[c].consistency_only]      # the end-to-end cases; rk4 is compared with itself only
STEPS = [(c, k) for c in CASES for k in CASES[c].nsteps]
COMPARED_STEPS = [(c, k) for c, k in STEPS if c in COMPARED]
CONDIM_CASES = {1: "rows1", 3: "types", 4: "rows4", 6: "rows6"}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# zone tables and contact lists in the reference's terms
def zone_table(model):
    t = model.tables
    return dict(body=np.asarray(t["touch_body"]).reshape(-1).astype(int), type=np.asarray(t["touch_type"]).reshape(-1).astype(int),
                pos=np.asarray(t["touch_pos"], dtype=np.float64).reshape(-1, 3), quat=np.asarray(t["touch_quat"], dtype=np.float64).reshape(-1, 4),
                size=np.asarray(t["touch_size"], dtype=np.float64).reshape(-1, 3))


def zones_at(model, xpos, xquat):
    """the zone table of the reference: the compiled zones (checked against the scene's intent in tests/test_cpu_touch.py) on bodies at xpos / xquat"""
    z = zone_table(model)
    pos, mat = R.zone_world_poses(z["body"], z["pos"], z["quat"], xpos, xquat)
    return dict(body=z["body"], type=z["type"], pos=pos, mat=mat, size=z["size"])


def contact_table(model, geom, pos, normal, force, efc_address):
    gb = np.asarray(model.tables["geom_bodyid"]).reshape(-1).astype(int)
    geom = np.asarray(geom, dtype=int).reshape(-1, 2)
    return dict(body=gb[geom], pos=pos, normal=normal, force=force, rows=np.asarray(efc_address).reshape(-1) >= 0)


_WORLDS = {}


def oracle_world(name, i, nstep, qpos=None):
    """world i of a case after forward() (nstep 0) or step(nstep) on the oracle, and the reference applied to the ORACLE's contacts, forces and body poses: dict(sensordata
    the oracle's own readings, counted [nz, nc] the oracle's own hit set, ncon, nefc, xpos, xquat, con (sim_contact_cases.read_contacts), ref [nz], info).  Cached: read only."""
    key = (name, i, nstep)
    if qpos is None and key in _WORLDS:
        return _WORLDS[key]
    case = CASES[name]
    got = S.oracle_world(case.scene, case.states, i, nstep, qpos=qpos)
    sim = S._oracle(case.scene)
    con = K.read_contacts(case.scene, sim)
    out = dict(sensordata=np.asarray(got["sensordata"]).copy(), counted=sim.touch_counted(), ncon=got["ncon"], nefc=got["nefc"], xpos=got["xpos"], xquat=got["xquat"], con=con)
    out["ref"], out["info"] = R.touch_reference(zones_at(case.model, got["xpos"], got["xquat"]),
                                                contact_table(case.model, con["contact_geom"], con["contact_pos"], con["contact_frame"][:, :3], con["contact_force"][:, 0], con["contact_efc_address"]))
    if qpos is None:
        _WORLDS[key] = out
    return out


def oracle_reference(name, nstep):
    """[n, ntouch]: the reference on the oracle's data, world by world"""
    return np.stack([oracle_world(name, i, nstep)["ref"] for i in range(CASES[name].n)])


def self_reference(model, xpos, xquat, geom, pos, normal, force, efc_address):
    """one world: (reference reading [nz], sum of the |normal forces| of the contacts that involve each zone's body [nz]) from an engine's OWN contact outputs of one pass"""
    ref, info = R.touch_reference(zones_at(model, xpos, xquat), contact_table(model, geom, pos, normal, force, efc_address))
    return ref, (info["involved"] * np.abs(np.asarray(force, dtype=np.float64))[None, :]).sum(axis=1), info


def pair_geoms(model, pair):
    g1, g2 = (np.asarray(model.tables[k]).reshape(-1) for k in ("pair_geom1", "pair_geom2"))
    pair = np.asarray(pair, dtype=int)
    return np.stack([g1[pair], g2[pair]], axis=1).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# recorded figures (tests/golden/touch_errors.json)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "touch_errors.json")
RATIO_MARGIN = 4.0


def golden():
    import json

    with open(GOLDEN) as fh:
        return json.load(fh)


def ratio_bound():
    """k of the self-consistency bound |sensordata - reference on the engine's own contacts| <= k eps32 sum |fn|: 4 x the largest ratio measured on the emulator (host build)"""
    return RATIO_MARGIN * golden()["self_consistency_ratio"]["emulator"]


def record(kind, end_to_end, ratio, counts=None):
    """with GRX_RECORD_TOUCH_ERRORS set: this run's worst end-to-end error per case and worst self-consistency ratio under `kind` ("emulator" or "mi355x")"""
    import json

    if not os.environ.get("GRX_RECORD_TOUCH_ERRORS"):
        return
    doc = golden() if os.path.exists(GOLDEN) else {}
    doc["bound"] = "end to end: |sensordata - touch_reference(oracle contacts)| <= %g absolute, every sensor of every case; self consistency: |sensordata - touch_reference(own contacts)| <= k eps32 sum |fn|, k = %g x the emulator's ratio" % (C.BOUND, RATIO_MARGIN)
    if end_to_end:      # empty when the end-to-end tests were deselected: the recorded rows stay
        doc.setdefault("end_to_end", {})[kind] = {k: float("%.3g" % v) for k, v in sorted(end_to_end.items())}
    doc.setdefault("self_consistency_ratio", {})[kind] = float("%.3g" % ratio)
    if counts:
        doc["counts"] = counts
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
