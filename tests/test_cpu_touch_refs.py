"""tests/touch_refs.py against itself: the interval-clipping decision of "the half line meets the solid zone" against a dense sampling of the ray with a point-in-solid
test, on a few thousand random (zone, ray) pairs per zone type -- origins inside, origins outside aimed at, away from and beside the zone, axis-parallel rays, rays along
the cylinder's axis -- and the summation rules of touch_reference on a hand-made contact list.

The sampling route shares nothing with the decision but the solid's defining inequalities.  It can only be trusted where the answer does not hinge on less than its step:
a pair is compared when the reference's own margin exceeds STEP, and most pairs must be."""
import numpy as np
import pytest

import touch_refs as R

PAIRS = 3000
STEP = 2.5e-4      # metres between two samples of a ray
REACH = 0.5        # the sampled length: the zones are within 0.2 m of every origin
SIZES = {R.SPHERE: (0.03, 0.0, 0.0), R.BOX: (0.03, 0.02, 0.012), R.CYLINDER: (0.025, 0.015, 0.0)}


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def make_pairs(kind, seed=0):
    rng = np.random.default_rng([0x70C4, kind, seed])
    size = np.array(SIZES[kind])
    n = PAIRS
    p, d = np.zeros((n, 3)), np.zeros((n, 3))
    q = n // 6
    p[:q] = rng.uniform(-1, 1, (q, 3)) * (size if kind == R.BOX else np.r_[size[0], size[0], size[1]] if kind == R.CYLINDER else size[0]) * 0.95      # near or inside the solid
    d[:q] = _unit(rng, q)
    o = _unit(rng, n - q) * rng.uniform(0.035, 0.15, (n - q, 1))      # outside the bounding sphere (0.038 at most) or close to it
    p[q:] = o
    aim = rng.uniform(-1.6, 1.6, (n - q, 3)) * np.maximum(size, size[0] if kind != R.BOX else 0.0)      # a point in or around the solid
    d[q:] = aim - o
    away = slice(2 * q, 3 * q)
    d[away] = -d[away]      # pointing away: a wrong sign would hit
    ax = slice(3 * q, 4 * q)      # axis-parallel rays from in front of a face, inside and outside its outline
    k = rng.integers(0, 3, q)
    p[ax] = rng.uniform(-1.5, 1.5, (q, 3)) * np.maximum(size, size[0] if kind != R.BOX else 0.0)
    p[ax][np.arange(q), k] = 0.0
    e = np.zeros((q, 3))
    e[np.arange(q), k] = rng.choice([-1.0, 1.0], q)
    p[ax] = p[ax] - e * rng.uniform(-0.01, 0.08, (q, 1))
    d[ax] = e * rng.uniform(0.5, 2.0, (q, 1))
    zs = slice(4 * q, 5 * q)      # along the cylinder's axis (z), both ways
    d[zs] = np.c_[np.zeros((q, 2)), rng.choice([-1.0, 1.0], q)]
    p[zs] = np.c_[rng.uniform(-1.6, 1.6, (q, 2)) * size[0], rng.uniform(-0.08, 0.08, q)]
    d *= rng.uniform(0.3, 3.0, (n, 1)) / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)      # of any length
    return size, p, d


def sampled(kind, size, p, d):
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    ts = np.arange(0.0, REACH, STEP)
    out = np.zeros(len(p), dtype=bool)
    for lo in range(0, len(ts), 250):
        x = p[:, None, :] + ts[None, lo:lo + 250, None] * u[:, None, :]
        out |= R.inside(kind, size, x).any(axis=1)
    return out


@pytest.mark.parametrize("kind", [R.SPHERE, R.BOX, R.CYLINDER])
def test_decision_equals_dense_sampling(kind):
    size, p, d = make_pairs(kind)
    hit = R.meets(kind, size, p, d)
    s = R.min_sdf(kind, size, p, d)
    firm = np.abs(s) > 2 * STEP
    want = sampled(kind, size, p, d)
    inside0 = R.inside(kind, size, p)
    print(R.TYPE_NAMES[kind], f"pairs {len(p)}, firm {int(firm.sum())}, hits {int((hit & firm).sum())}, misses {int((~hit & firm).sum())}, origins inside {int((inside0 & firm).sum())}")
    assert firm.mean() > 0.8 and (hit & firm).sum() > 300 and (~hit & firm).sum() > 300 and (inside0 & firm).sum() > 100
    assert inside0[hit != want].sum() == 0 and (hit[firm] == want[firm]).all(), np.nonzero(firm & (hit != want))[0]
    assert hit[inside0].all()      # an origin inside the zone hits, whatever the direction
    assert ((s < 0) == hit)[np.abs(s) > 1e-9].all()      # the distance minimum is a second decision
    # moving a ray by less than its margin does not flip the decision
    rng = np.random.default_rng(kind)
    shift = _unit(rng, len(p)) * (0.9 * np.abs(s))[:, None]
    assert (R.meets(kind, size, p + shift, d) == hit)[np.abs(s) > 1e-9].all()


def test_the_length_of_the_direction_does_not_matter():
    for kind in (R.SPHERE, R.BOX, R.CYLINDER):
        size, p, d = make_pairs(kind, seed=1)
        assert (R.meets(kind, size, p, d) == R.meets(kind, size, p, 7.0 * d)).all()
        assert np.abs(R.min_sdf(kind, size, p, d) - R.min_sdf(kind, size, p, 0.01 * d)).max() < 1e-9


def test_hand_made_rays():
    z = np.array([0.0, 0.0, 1.0])
    for kind, size in ((R.SPHERE, (0.01, 0, 0)), (R.BOX, (0.01, 0.01, 0.01)), (R.CYLINDER, (0.01, 0.01, 0))):
        m = lambda p, d: bool(R.meets(kind, size, np.array([p], dtype=float), np.array([d], dtype=float))[0])
        assert m([0, 0, -0.05], z) and not m([0, 0, -0.05], -z) and not m([0.02, 0, -0.05], z) and m([0.002, 0.001, 0.003], -z) and m([0.002, 0.001, 0.003], [1, 0, 0])
        assert not m([0, 0, 0.011], z) and m([0, 0, 0.011], -z)
        s = R.min_sdf(kind, size, np.array([[0, 0, -0.05], [0.02, 0, -0.05], [0, 0, 0.05]], dtype=float), np.array([z, z, z]))
        assert np.allclose(s, [-0.01, 0.01, 0.04], atol=1e-9), s


def test_touch_reference_counts_what_the_definition_counts():
    eye = np.eye(3)
    zones = dict(body=[1, 1, 2, 3], type=[R.BOX, R.SPHERE, R.CYLINDER, R.BOX], pos=[[0, 0, 0], [0, 0, 0.1], [0, 0, -0.02], [0, 0, 0]], mat=[eye] * 4,
                 size=[[0.05, 0.05, 0.01], [0.01, 0, 0], [0.01, 0.01, 0], [1, 1, 1]])
    con = dict(body=[[0, 1], [0, 1], [1, 2], [0, 1], [0, 1], [2, 1]],
               pos=[[0.04, 0.04, 0], [-0.04, 0.04, 0], [0, 0, 0.03], [0.2, 0, 0], [0.0, 0.0, 0.0], [0, 0, 0.03]],
               normal=[[0, 0, 1]] * 3 + [[0, 0, 1], [0, 0, 1], [0, 0, -1]], force=[1.0, 2.0, 4.0, 8.0, 16.0, 32.0], rows=[True, True, True, True, False, True])
    val, info = R.touch_reference(zones, con)
    # zone 0 (body 1): contacts 0, 1 inside; contact 2 (body 1 first, ray up from z = 0.03: away); 3 beside; 4 has no rows; 5 (body 1 second: the ray -(-z) = +z, away)
    # zone 1 (body 1, sphere at z = 0.1): contact 2 ray up from 0.03 hits; contact 5 too (second body, normal down, ray up); 0 and 1 are second body with normal up: ray down, miss
    # zone 2 (body 2, cylinder at z = -0.02): contact 2 (second body: ray down from 0.03) hits, contact 5 (first body, normal down) hits
    # zone 3 (body 3): no contact involves it
    assert val.tolist() == [3.0, 36.0, 36.0, 0.0], val
    assert info["involved"].sum(axis=1).tolist() == [6, 6, 2, 0] and not info["counted"][:, 4].any() and info["hit"][0, 4]
    assert np.isinf(info["margin"][3]).all() and np.isfinite(info["margin"][0]).all()
    con["force"][0] = 0.0      # a force that is not > 0 is not counted
    assert R.touch_reference(zones, con)[0][0] == 2.0


def test_zone_world_poses():
    q = np.array([0.5, 0.5, 0.5, 0.5])      # x -> y -> z -> x
    c, M = R.zone_world_poses([1], [[1.0, 0, 0]], [[1.0, 0, 0, 0]], [[0, 0, 0], [0, 0, 2.0]], [[1, 0, 0, 0], q])
    assert np.allclose(c, [[0, 1, 2]]) and np.allclose(M[0] @ [1, 0, 0], [0, 1, 0])
