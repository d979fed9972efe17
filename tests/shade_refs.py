"""The fp64 reference of the colour / surface-normal cameras (BatchedSim.render(rgb=True, normals=True), grx_sim_render_rgb): the outward normal at a hit and the shaded
RGBA8 pixel, written from the definition in include/grx_capi.h and sharing no code with csrc/grx_shade.h.  The hit itself, (dist, geom), is ray_cases.cast()'s."""
import numpy as np

import ray_cases as R

_unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)


def local_normal(kind, size, planes, x):
    """outward unit normals [n, 3] at the surface points x [n, 3], both in the geom's frame; a surface with faces: the face x lies nearest, the smaller index on a tie"""
    zero, rows = 0.0 * x[:, 0], np.arange(len(x))
    if kind == 3:
        return _unit(x - np.stack([zero, zero, np.clip(x[:, 2], -size[1], size[1])], axis=1))
    if kind in (2, 4):      # a sphere: x; an ellipsoid: (x / a^2, y / b^2, z / c^2)
        return _unit(x / size ** 2 if kind == 4 else x)
    if kind == 5:
        cap = np.abs(np.abs(x[:, 2]) - size[1]) <= np.abs(np.hypot(x[:, 0], x[:, 1]) - size[0])
        return np.where(cap[:, None], np.stack([zero, zero, np.where(x[:, 2] < 0, -1.0, 1.0)], axis=1), _unit(np.stack([x[:, 0], x[:, 1], zero], axis=1)))
    if kind == 7:
        return planes[np.argmin(np.abs(x @ planes[:, :3].T - planes[:, 3]), axis=1), :3]
    n, face = np.zeros_like(x), np.argmin(np.abs(np.abs(x) - size), axis=1) if kind == 6 else np.full(len(x), 2)      # (argmin: the first of equal values); a plane: +z
    n[rows, face] = np.where((x[rows, face] < 0) & (kind == 6), -1.0, 1.0)
    return n


def normals(model, gxpos, gxmat, o, d, dist, geom):
    """world-frame outward unit normals [n, 3] at the hits (dist, geom) of the rays o, d [n, 3]; a miss: 0"""
    G, gxpos, gxmat, out = R.geoms_of(model), np.asarray(gxpos).reshape(-1, 3), np.asarray(gxmat).reshape(-1, 3, 3), np.zeros((len(o), 3))
    for g in np.unique(geom[geom >= 0]):
        x = (o[geom == g] + dist[geom == g, None] * d[geom == g] - gxpos[g]) @ gxmat[g]
        out[geom == g] = local_normal(G.type[g], G.size[g], G.planes.get(g), x) @ gxmat[g].T
    return out


def shade(n, d, geom, colors, ambient=0.3, diffuse=0.7, sun=None, sun_diffuse=0.5, background=(0.0, 0.0, 0.0)):
    """RGBA levels [n, 4] (ints 0 .. 255) of the pixels with normals n, ray directions d and winners geom; colors [ngeom, 3]"""
    level, nv = lambda x: np.floor(255.0 * np.clip(x, 0.0, 1.0) + 0.5).astype(int), -(n * _unit(d)).sum(1)
    s = ambient + diffuse * np.abs(nv)
    if sun is not None:
        s = s + sun_diffuse * np.maximum(0.0, np.where(nv < 0, -1.0, 1.0) * -(n @ _unit(np.asarray(sun, dtype=np.float64))))
    out = np.concatenate([level(np.clip(np.asarray(colors, dtype=np.float64), 0.0, 1.0)[np.maximum(geom, 0)] * s[:, None]), np.full((len(n), 1), 255)], axis=1)
    out[geom < 0] = list(level(np.asarray(background, dtype=np.float64))) + [0]
    return out
