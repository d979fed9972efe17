"""fp64 reference of the body wrenches of grx.BatchedSim (body_dynamics=): subtree_com, cfrc_ext, cacc and cfrc_int of a tests/dyn_tree_cases.py tree without contacts, from
the definitions -- no cdof, no spatial algebra.  Per tree body e the classical Newton-Euler quantities at its centre of mass, F_e = m_e (a_com - g) and N_e = I_e alpha +
omega x I_e omega, with a, alpha, omega from sensor_refs.evaluate on one synthetic xbody framelinacc / frameangacc / frameangvel / framelinvel set per body, shifted rigidly.
Rows are the COMPILED model's bodies (`rows`: their names, row 0 the world): a joint-less tree body has none and counts towards the nearest ancestor that has one, so an
applied wrench (f, t) on row b acts at the centre of mass of b's group, the compiled xipos.  cfrc_int[b] = sum over the tree bodies below b of
[(N_e - t_e) + (x_e - c) x (F_e - f_e); F_e - f_e] about c = subtree_com[root(b)]; cacc_lin[b] = a(c) - omega x u(c) of the point of b at c.  `err`: the reference's own error
estimate per output, the sensor reference's estimates and that of qacc carried through the same sums in absolute values."""
import numpy as np

import dyn_refs as R
import sensor_refs as SR

_TYPES = ("framelinacc", "frameangacc", "frameangvel", "framelinvel")


def evaluate(tree, q, v, rows, applied=None):
    """rows: compiled body names, rows[0] the world.  applied: {row name: (f [3], t [3])}.  dict(subtree_com [nr, 3], cfrc_ext / cacc / cfrc_int [nr, 6], mass, err {...})"""
    bodies, applied = tree["bodies"], dict(applied or {})
    nb, names = len(bodies), [b["name"] for b in tree["bodies"]]
    ev, kin, anc = R.evaluate(tree, q, v), R.kinematics(tree, q), R.ancestors(tree)
    mass, x, g = np.array([b["mass"] for b in bodies], dtype=np.float64), kin["xipos"], np.asarray(tree["gravity"], dtype=np.float64)
    row_of = np.array([max((a for a in np.nonzero(anc[e])[0] if names[a] in rows), key=lambda a: anc[a].sum()) for e in range(nb)])      # the group a tree body counts towards
    root = np.array([min(np.nonzero(anc[e])[0], key=lambda a: anc[a].sum()) for e in range(nb)])
    point = {b: (mass[row_of == b] @ x[row_of == b]) / mass[row_of == b].sum() for b in set(row_of)}      # compiled xipos
    Q = np.zeros(len(ev["qacc"]))
    for name, (f, t) in applied.items():
        jp, jr = R.jacobians(tree, kin, point[names.index(name)][None], [names.index(name)])
        Q += jp[0].T @ f + jr[0].T @ t
    qacc = np.linalg.solve(ev["M"], ev["qfrc_smooth"] + Q)
    sensors = [dict(name=f"{t}{e}", type=t, objtype="xbody", objname=names[e], cutoff=0.0) for e in range(nb) for t in _TYPES]
    sr = SR.evaluate(tree, q, v, sensors, qacc=qacc)
    jp0, jr0 = R.jacobians(tree, kin, kin["xpos"], np.arange(nb))
    qe = np.asarray(ev["err"]["qacc"]) * np.ones(len(qacc))
    data = sr["data"].reshape(nb, 4, 3)
    err = sr["err"].reshape(nb, 4, 3) + np.stack([np.abs(jp0) @ qe, np.abs(jr0) @ qe, np.zeros((nb, 3)), np.zeros((nb, 3))], axis=1)
    a0, al, om, u0 = (data[:, k] for k in range(4))
    xc = lambda a, b: np.cross(np.abs(a), np.abs(b)) + 2.0 * np.abs(a)[..., [2, 0, 1]] * np.abs(b)[..., [1, 2, 0]]      # |a x b| <= this, componentwise
    at = lambda p: (a0 + np.cross(al, p - kin["xpos"]) + np.cross(om, np.cross(om, p - kin["xpos"])), err[:, 0] + xc(err[:, 1], p - kin["xpos"]))      # (a - g, its error) of the body points p
    (ac, ace), Iw = at(x), ev["Iw"]
    F, Fe = mass[:, None] * ac, mass[:, None] * ace
    Nn, Ne = np.einsum("bkl,bl->bk", Iw, al) + np.cross(om, np.einsum("bkl,bl->bk", Iw, om)), np.einsum("bkl,bl->bk", np.abs(Iw), err[:, 1])
    sub = lambda b: anc[:, b] if b >= 0 else np.ones(nb, dtype=bool)
    com = lambda b: mass[sub(b)] @ x[sub(b)] / mass[sub(b)].sum()
    nr = len(rows)
    out = dict(subtree_com=np.zeros((nr, 3)), cfrc_ext=np.zeros((nr, 6)), cacc=np.zeros((nr, 6)), cfrc_int=np.zeros((nr, 6)), mass=float(mass.sum()))
    oe = {k: np.zeros_like(out[k]) for k in ("cacc", "cfrc_int")}
    for r, name in enumerate(rows):
        b = names.index(name) if r else -1
        c = com(root[b]) if r else com(-1)
        out["subtree_com"][r] = com(b)
        if r:
            (acp, acpe), d = at(np.tile(c, (nb, 1))), c - kin["xpos"][b]
            out["cacc"][r] = np.concatenate([al[b], acp[b] - np.cross(om[b], u0[b] + np.cross(om[b], d))])
            oe["cacc"][r] = np.concatenate([err[b, 1], acpe[b] + xc(om[b], err[b, 3])])
            if name in applied:
                f, t = applied[name]
                out["cfrc_ext"][r] = np.concatenate([t + np.cross(point[b] - c, f), f])
        else:
            out["cacc"][r, 3:] = -g
        for e in np.nonzero(sub(b))[0]:
            out["cfrc_int"][r] += np.concatenate([Nn[e] + np.cross(x[e] - c, F[e]), F[e]])
            oe["cfrc_int"][r] += np.concatenate([Ne[e] + xc(x[e] - c, Fe[e]), Fe[e]])
        for n, (f, t) in applied.items():
            if sub(b)[names.index(n)]:
                out["cfrc_int"][r] -= np.concatenate([t + np.cross(point[names.index(n)] - c, f), f])
    out["err"] = dict(oe, subtree_com=float(ev["err"]["xipos"]), cfrc_ext=float(ev["err"]["xipos"]) * (1.0 + max((float(np.abs(f).max()) for f, _ in applied.values()), default=0.0)))
    return out
