"""Touch sensors zone by zone without a GPU: the preconditions of every comparison of tests/touch_cases.py on the oracle and the reference alone, the oracle's own touch
routine against the reference, what the committed tables cover, and the generic engine's grx_touch_sensors on the emulator (host build of the kernel source):
end to end against the reference on the oracle's contacts, against the reference on its own contacts (which fixes the k of the self-consistency bound), and modes 2 - 4."""
import types

import numpy as np
import pytest

import engine_matrix_cases as C
import sim_cases as S
import touch_cases as T
import touch_refs as R

_EMU = {}
_WORST = {}


def emu_of(name):
    if name not in _EMU:
        from emu_sim import EmuSim

        _EMU[name] = EmuSim(T.CASES[name].model, types.SimpleNamespace(obs_dim=1))
    return _EMU[name]


def emu_world(name, i, nstep, mode=1):
    case, e = T.CASES[name], emu_of(name)
    st = case.states
    e.qpos[:], e.qvel[:] = st["qpos"][i], st["qvel"][i]
    return e.touch(mode=mode, nstep=nstep)


# the scenes are what they say ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.CASES))
def test_compiled_zone_tables_match_the_scene(name):
    """touch_body / type / pos / quat / size of the compiled model against the zone table the scene was generated from, which gives each zone's pose on the body that
    survives compilation: the compiler's composition of a static child's pose is checked against the intent, not against itself"""
    case = T.CASES[name]
    z = T.zone_table(case.model)
    assert len(z["body"]) == len(case.zones) and list(case.model.names["touch"]) == ["t_" + w["name"] for w in case.zones]
    for k, want in enumerate(case.zones):
        assert z["body"][k] == case.model.names["body"][want["body"]] and z["type"][k] == want["type"], (name, want["name"])
        used = {R.SPHERE: 1, R.CYLINDER: 2, R.BOX: 3}[want["type"]]      # the size components the type reads (the others keep the site's default)
        assert np.abs(z["pos"][k] - want["pos"]).max() < 1e-12 and (z["size"][k][:used] == want["size"][:used]).all(), (name, want["name"], z["pos"][k], want["pos"])
        assert np.abs(R.quat_to_mat(z["quat"][k]) - R.quat_to_mat(want["quat"])).max() < 1e-12, (name, want["name"])
    if name == "types":
        assert sum(w["child"] is not None for w in case.zones) == 12 and "plate" not in case.model.names["body"]      # the child was merged
    if name == "grid70":
        assert len(case.zones) == 70


# well-posedness: a precondition, on the oracle and the reference alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nstep", T.STEPS)
def test_every_decision_is_well_posed(name, nstep):
    """no case and no world is left out: every (zone, contact) decision has a margin of at least 1 mm, every counted force is at least 0.05 N, and the oracle's answer
    moves less than SENS_MAX under the one-ulp jitter of the start"""
    case = T.CASES[name]
    margin, force = np.inf, np.inf
    for i in range(case.n):
        w = T.oracle_world(name, i, nstep)
        inv = w["info"]["involved"]
        rows = w["con"]["contact_efc_address"] >= 0
        if inv.any():
            margin = min(margin, w["info"]["margin"][inv].min())
        f = np.broadcast_to(w["con"]["contact_force"][:, 0], inv.shape)[w["info"]["counted"]]
        if f.size:
            force = min(force, f.min())
        live = np.broadcast_to(w["con"]["contact_force"][:, 0] > 0, inv.shape) & inv & rows[None, :]
        assert (np.broadcast_to(w["con"]["contact_force"][:, 0], inv.shape)[live] >= T.MIN_FORCE).all(), (name, i, "a force between 0 and MIN_FORCE decides a reading")
    sens = S.oracle_sensitivity(case.scene, case.n, nstep)
    print(f"{name} nstep={nstep}: smallest margin {1e3 * margin:.2f} mm, smallest counted force {force:.3f} N, oracle sensitivity {sens.max():.1e}")
    assert margin >= T.MIN_MARGIN and force >= T.MIN_FORCE and (sens < C.SENS_MAX).all(), (name, nstep, margin, force, sens)


# 4b: the oracle's own touch against the reference on its own contacts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nstep", T.STEPS)
def test_oracle_touch_equals_the_reference(name, nstep):
    case = T.CASES[name]
    worst = 0.0
    for i in range(case.n):
        w = T.oracle_world(name, i, nstep)
        assert w["counted"].shape == w["info"]["counted"].shape and (w["counted"] == w["info"]["counted"]).all(), (name, i, "hit sets", np.argwhere(w["counted"] != w["info"]["counted"]))
        rel = np.abs(w["sensordata"] - w["ref"]) / np.maximum(np.abs(w["ref"]), 1e-300)
        rel[(w["ref"] == 0) & (w["sensordata"] == 0)] = 0.0
        worst = max(worst, rel.max())
    print(f"{name} nstep={nstep}: hit sets equal, worst relative difference {worst:.1e}")
    assert worst <= 1e-12


# what the committed tables cover, asserted on the reference ---------------------------------------------------------------------------------------------------------
def _flipped_decisions(name, i, nstep):
    """[nz, nc]: the reference's decisions with every ray reversed, and whether each ray's origin lies inside the zone"""
    w = T.oracle_world(name, i, nstep)
    case = T.CASES[name]
    con = w["con"]
    tab = T.contact_table(case.model, con["contact_geom"], con["contact_pos"], -con["contact_frame"][:, :3], con["contact_force"][:, 0], con["contact_efc_address"])
    z = T.zones_at(case.model, w["xpos"], w["xquat"])
    _, rev = R.touch_reference(z, tab)
    inside = np.array([[R.inside(z["type"][k], z["size"][k], (p - z["pos"][k]) @ z["mat"][k]) for p in con["contact_pos"]] for k in range(len(z["body"]))]).reshape(rev["hit"].shape)
    return rev["hit"], inside


def test_coverage_placements_of_every_zone_type():
    """types: each of the four placements for each of the three zone types, on the ball and on its merged child, in every world"""
    case = T.CASES["types"]
    for nstep in case.nsteps:
        for i in range(case.n):
            w = T.oracle_world("types", i, nstep)
            rev, inside = _flipped_decisions("types", i, nstep)
            assert w["ncon"] == 1 and w["con"]["contact_force"][0, 0] > T.MIN_FORCE
            seen = set()
            for k, z in enumerate(case.zones):
                kind, pl = z["tag"]
                hit, back, ins = w["info"]["hit"][k, 0], rev[k, 0], inside[k, 0]
                assert (hit, back, ins) == {"in": (True, True, True), "hit": (True, False, False), "away": (False, True, False), "beside": (False, False, False)}[pl], (z["name"], hit, back, ins)
                seen.add((z["child"] is not None, kind, pl))
            assert len(seen) == 24


def test_coverage_both_body_orders():
    """the A - B contact lists A's geom first in one scene and second in the other, so every zone's body is a contact's first body once and its second body once"""
    first = {}
    for name in ("order-ab", "order-ba"):
        case = T.CASES[name]
        a, b = case.model.names["geom"]["Ag"], case.model.names["geom"]["Bg"]
        for i in range(case.n):
            g = T.oracle_world(name, i, 0)["con"]["contact_geom"]
            ab = [tuple(r) for r in g if set(r) == {a, b}]
            assert len(ab) == 1
            first.setdefault(name, set()).add("A" if ab[0][0] == a else "B")
    print("first geom of the A - B contact:", first)
    assert first["order-ab"] != first["order-ba"] and all(len(v) == 1 for v in first.values())
    for name in ("order-ab", "order-ba", "both"):      # one contact feeds a zone on each body
        for i in range(T.CASES[name].n):
            w = T.oracle_world(name, i, 0)
            names = [z["name"] for z in T.CASES[name].zones]
            fed = {n: w["ref"][names.index(n)] for n in names}
            assert fed["a_in"] > 0 and fed["a_in"] == fed["a_hit"] == fed["b_in"] == fed["b_hit"] and fed["a_away"] == fed["b_away"] == fed["a_beside"] == fed["b_beside"] == 0
            assert fed["b_floor"] > 0 and fed["b_floor"] == fed["b_under"] and fed["b_floor"] != fed["b_in"]


def test_coverage_rows():
    for dim, name in T.CONDIM_CASES.items():
        for i in range(T.CASES[name].n):
            con = T.oracle_world(name, i, 0)["con"]
            assert con["contact_dim"].tolist() == [dim] and con["contact_efc_address"][0] >= 0
            assert T.oracle_world(name, i, 0)["nefc"] == {1: 1, 3: 4, 4: 6, 6: 10}[dim]
    for nstep in (0, 1):      # the contact inside the gap: listed, without rows, and nothing reads it
        w = T.oracle_world("gap", 0, nstep)
        ball = T.CASES["gap"].model.names["geom"]["ballg"]
        k = [j for j, g in enumerate(w["con"]["contact_geom"]) if ball in g]
        assert len(k) == 1 and w["con"]["contact_efc_address"][k[0]] < 0 and w["ncon"] == 2 and w["nefc"] == 4
        assert w["info"]["hit"][:24, k[0]].sum() >= 6 and (w["ref"][:24] == 0).all() and w["ref"][24] > T.MIN_FORCE


def test_coverage_axes_many_and_grid():
    for i in range(T.CASES["axes"].n):
        w = T.oracle_world("axes", i, 0)
        assert w["ncon"] == 4
        for k, z in enumerate(T.CASES["axes"].zones):
            assert (w["ref"][k] > 0) == (z["tag"] in ("in", "hit")), z["name"]
            assert w["info"]["hit"][k].sum() == (1 if z["tag"] in ("in", "hit") else 0)
    st = T.CASES["axes"].states
    assert st["qpos"][0, 3:7].tolist() == [1.0, 0.0, 0.0, 0.0]      # world 0: the ray is exactly (0, 0, -1) in every zone frame
    case = T.CASES["many"]
    names = [z["name"] for z in case.zones]
    from gymnasium_robotics_amd.core import RERUN_CAPACITY

    for nstep in (0, 1):
        for i in range(case.n):
            w = T.oracle_world("many", i, nstep)
            f = np.sort(w["con"]["contact_force"][:4, 0])
            down = i in T.MANY_DOWN
            assert w["ncon"] == (9 if down else 4) and (w["ncon"] > T.MANY_CAPACITY["maxcon"]) == down and w["ncon"] <= RERUN_CAPACITY["maxcon"] and w["nefc"] <= T.MANY_CAPACITY["maxefc"]
            hits = {n: int(w["info"]["counted"][names.index(n)].sum()) for n in names}
            assert (hits["pad2"], hits["pad4"], hits["pad1"], hits["pad_diag"], hits["pad_top"]) == (2, 4, 1, 2, 0), hits
            assert all(hits[f"ball{k}_zone"] == (1 if down else 0) for k in range(T.MANY_BALLS))
            assert all((w["ref"][names.index(f"ball{k}_zone")] == 0) == (not down) for k in range(T.MANY_BALLS))
            assert np.diff(f).min() > 1e-3      # four different forces: a sum over the wrong two of them is a different number
    case = T.CASES["grid70"]
    for nstep in (0, 1):
        for i in range(case.n):
            w = T.oracle_world("grid70", i, nstep)
            live = np.nonzero(w["ref"] > 0)[0]
            assert w["ncon"] == 4 and sorted(live.tolist()) == [0, 1, 8, 9, 60, 61, 68, 69], live
            assert (w["ref"][[68, 69]] > T.MIN_FORCE).all()      # readings at zone indices >= 64: the second trip of the lane loop
            _, inside = _flipped_decisions("grid70", i, nstep)
            assert inside[[0, 9, 60, 69]].sum() == 4 and inside[[1, 8, 61, 68]].sum() == 0      # the corner zones contain their contact, the low rows are hit from outside


# 4a on the emulator ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.COMPARED)
def test_emulator_equals_the_reference_on_the_oracle_contacts(name):
    case = T.CASES[name]
    worst = 0.0
    for nstep in case.nsteps:
        want = T.oracle_reference(name, nstep)
        for i in range(case.n):
            got, w = emu_world(name, i, nstep), T.oracle_world(name, i, nstep)
            err = np.abs(got["sensordata"].astype(np.float64) - want[i])
            worst = max(worst, err.max())
            print(f"{name} nstep={nstep} world {i}: worst error {err.max():.2e}, ncon {got['ncon']} nefc {got['nefc']}")
            assert (got["ncon"], got["nefc"], got["status"] & 0xFFFF) == (w["ncon"], w["nefc"], 0), (name, nstep, i, got["ncon"], got["nefc"], got["status"])
            assert np.isfinite(got["sensordata"]).all() and (err <= C.BOUND).all(), (name, nstep, i, np.nonzero(~(err <= C.BOUND))[0], got["sensordata"], want[i])
            assert (got["sensordata"][want[i] == 0] == 0).all(), (name, nstep, i, "a zone no contact feeds must read exactly 0")
    _WORST[name] = worst


# 4c on the emulator: this is where k comes from ------------------------------------------------------------------------------------------------------------------------
def test_emulator_sensordata_equals_the_reference_on_its_own_contacts():
    """K12 alone: the reference applied to the emulator's OWN contact list, forces and body poses of the same pass leaves fp32 summation error only,
    |difference| <= k eps32 sum |fn| per sensor (the sum over the contacts that involve the zone's body).  The largest ratio seen here, times 4, is k."""
    ratio, checked = 0.0, 0
    for name, nstep in T.STEPS:
        case = T.CASES[name]
        for i in range(case.n):
            em = emu_world(name, i, nstep)
            ref, scale, info = T.self_reference(case.model, em["xpos"], em["xquat"], T.pair_geoms(case.model, em["pair"]), em["pos"], em["normal"], em["force"], em["efc_address"])
            d = np.abs(em["sensordata"].astype(np.float64) - ref)
            assert (d[scale == 0] == 0).all(), (name, nstep, i)
            if (scale > 0).any():
                ratio = max(ratio, float((d[scale > 0] / (T.EPS32 * scale[scale > 0])).max()))
            checked += int((scale > 0).sum())
    print(f"self consistency on the emulator: worst |difference| / (eps32 sum |fn|) = {ratio:.3f} over {checked} sensors")
    T.record("emulator", _WORST, ratio, counts=dict(cases=len(T.CASES), compared=len(T.COMPARED), worlds=sum(c.n for c in T.CASES.values()),
                                                   zones=sum(len(c.zones) for c in T.CASES.values())))
    assert ratio <= T.ratio_bound(), (ratio, T.ratio_bound())


# 4d: modes -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["types", "many"])
def test_emulator_modes(name):
    case = T.CASES[name]
    for nstep in case.nsteps:
        want = T.oracle_reference(name, nstep)
        for i in range(case.n):
            m2, m3, m4 = (emu_world(name, i, nstep, mode=m)["sensordata"].astype(np.float64) for m in (2, 3, 4))
            assert (m2 == (want[i] > 0)).all(), (name, nstep, i, m2, want[i])
            assert np.abs(m3 - np.log1p(want[i])).max() <= C.BOUND and np.abs(m4 - np.clip(want[i], -1.0, 1.0)).max() <= C.BOUND, (name, nstep, i)
        if name == "many":      # the clip of mode 4 acts on some readings and not on others
            assert (want > 1.0).any() and ((want > 0) & (want < 1.0)).any()
