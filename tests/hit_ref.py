"""The reference's hit frame -- TEST INFRASTRUCTURE ONLY.

The oracle (oracle/rt_oracle.c) returns colours; what `collide` found before
it shaded (MainState.cpp:330-394: the float `closest` and the object that set
it) is rebuilt here from the oracle's own per-primitive functions.  None of
the hit tests' arithmetic is restated: this module only holds the loop order
of `collide` -- every cube's twelve triangles in order, then every sphere in
order, each taken where it is strictly nearer than everything before it.
tests/test_hit_format.py pins the result to `oracle.trace` through the
library's `shade_hits`.
"""
import numpy as np

F32 = np.float32
REF_DIR = (0.0, 0.0, -1.0, -1.0)
K_FAR = F32(300000.0)  # MainState.cpp:345


def hit_dtype():
    return np.dtype([("t", "<f4"), ("object", "<i4")])


def hit_ref(oracle, scene, w, h, rows=None, ray_dir=REF_DIR, x_begin=0):
    """(rows x w) records (t, object) of the reference's implicit-origin
    frame: object = cube index, or num_cubes + sphere index, or -1 beside
    t = 300000 where nothing was hit.  `x_begin`: the frame column of the
    first of the `w` columns computed (a window of a wider frame)."""
    rb, re = rows if rows is not None else (0, h)
    n = re - rb
    d = np.ascontiguousarray(ray_dir, F32)
    closest = np.full((n, w), K_FAR, F32)
    obj = np.full((n, w), -1, np.int32)
    cubes = np.ascontiguousarray(scene.cube_vertices, F32).reshape(-1, 36, 4)
    for c in range(len(cubes)):
        for k in range(0, 36, 3):
            # intersectTri's fp64 t (NaN: no hit), then `(float)t < closest`
            t = oracle.tri_t_grid(cubes[c, k], cubes[c, k + 1], cubes[c, k + 2], d, x_begin,
                                  rb, w, n)
            with np.errstate(over="ignore", invalid="ignore"):
                tf = t.astype(F32)
                take = ~np.isnan(t) & (tf < closest)
            closest[take] = tf[take]
            obj[take] = c
    origins = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)
    radius = np.ascontiguousarray(scene.sphere_radius, F32).reshape(-1)
    for i in range(len(radius)):
        # pixels the sphere test does not leave early (everywhere else it
        # returns the 0 that collide skips)
        marked = oracle.sphere_grid(origins[i], radius[i], d, x_begin, rb, w, n)
        # oracle.intersect_sphere per marked pixel, without its per-call array
        # conversions (some directions mark every pixel of every sphere)
        org = np.array([0.0, 0.0, 0.0, 1.0], F32)
        call, po, pd, pc = (oracle.lib.orc_intersect_sphere, org.ctypes.data, d.ctypes.data,
                            origins[i].ctypes.data)
        r = float(radius[i])
        for y, x in zip(*np.nonzero(marked)):
            org[0], org[1] = x_begin + x, rb + y
            dist = F32(call(po, pd, r, pc))
            if dist == 0.0:
                continue
            if dist < closest[y, x]:
                closest[y, x] = dist
                obj[y, x] = len(cubes) + i
    out = np.empty((n, w), hit_dtype())
    out["t"] = closest
    out["object"] = obj
    return out


def words(hits):
    """A hit frame as its raw 32-bit words (rows x w x 2): NaN-safe, -0 != +0."""
    return np.ascontiguousarray(hits).view(np.uint32).reshape(hits.shape + (2,))


def distinct_colours(scene):
    """`scene` with every object given its own colour in [0.25, 1] (alpha
    255), so that a colour frame tells which object won a pixel."""
    n = len(scene.cube_colours) + len(scene.sphere_colours)
    i = np.arange(n, dtype=np.float64)
    col = np.stack([0.25 + 0.75 * ((i * 0.618033988749895) % 1.0),
                    0.25 + 0.75 * ((i * 0.381966011250105 + 0.3) % 1.0),
                    0.25 + 0.75 * ((i + 1.0) / (n + 1.0)),
                    np.full(n, 255.0)], axis=1).astype(F32)
    assert len({tuple(c) for c in col.tolist()}) == n
    nc = len(scene.cube_colours)
    return type(scene)(scene.sphere_origins.copy(), scene.sphere_radius.copy(), col[nc:],
                       scene.cube_vertices.copy(), col[:nc])
