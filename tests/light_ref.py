"""Surfaces and diffuse lighting of a hit frame -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of DESIGN.md §3.1a for rt_hit_surfaces / rt_light_hits.
Which of a cube's twelve triangles gave a pixel its t is found with the
oracle's own fp64 `tri_t_grid`, triangle by triangle in the reference's
order: no intersection arithmetic is restated.  Everything else is
elementwise `np.float32` arithmetic, one ufunc per written operation (numpy
never contracts), in the written order.
"""
import numpy as np

from gpu_support import H, W, base_scene
from hit_ref import K_FAR, REF_DIR, distinct_colours, hit_ref

F32 = np.float32
INT_MIN = -(1 << 31)
MINUS_INF_DIR = (0.0, 0.0, -1e-4, -1.0)
ONE_LIGHT = [(48, 40, 200, 1)]
THREE_LIGHTS = ONE_LIGHT + [(0, 0, 50, 1), (120, 90, -20, 1)]
_CACHE = {}


def surface_dtype():
    return np.dtype([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("triangle", "<i4")])


def with_lights(scene, lights):
    """`scene` with the given float4 lights (xyz position, w reserved)."""
    return type(scene)(scene.sphere_origins, scene.sphere_radius, scene.sphere_colours,
                       scene.cube_vertices, scene.cube_colours,
                       np.asarray(lights, F32).reshape(-1, 4))


def base(pkg):
    return distinct_colours(base_scene(pkg))


def one_sphere(pkg, origin, radius, colour):
    return pkg.Scene(np.array([origin], F32), np.array([radius], F32), np.array([colour], F32))


def one_cube(pkg, ops, colour):
    return pkg.Scene(cube_vertices=pkg.cube_packed(ops).reshape(1, 36, 4),
                     cube_colours=np.array([colour], F32))


def edge_scenes(pkg):
    """(key, scene, w, h, ray_dir): the base scene and the numeric edges of
    the shade (tests/test_hit_format.py): t = -inf, a channel past int32, a
    NaN colour."""
    return [
        ("base", base(pkg), W, H, REF_DIR),
        ("minus_inf", one_cube(pkg, [("scale", 20, 16, 1), ("translate", 16, 12, 3e38)],
                               (1, 0.5, 0.0, 255)), 32, 24, MINUS_INF_DIR),
        ("past_int32", one_sphere(pkg, (16, 12, -10, 1), 2e9, (1.0, 0.25, -0.25, 255)), 32, 24,
         REF_DIR),
        ("nan_colour", one_sphere(pkg, (16, 12, -50, 1), 9, (np.nan, 0.5, 1.0, 255)), 32, 24,
         REF_DIR),
    ]


def cached_hits(oracle, key, scene, w, h, rows=None, ray_dir=REF_DIR, x_begin=0):
    """hit_ref, computed once per key and read-only.  (The key holds the
    direction's words: -0.0 and 0.0 are different frames' keys.)"""
    k = ("hits", key, w, h, rows, np.asarray(ray_dir, F32).tobytes(), x_begin)
    if k not in _CACHE:
        r = hit_ref(oracle, scene, w, h, rows=rows, ray_dir=ray_dir, x_begin=x_begin)
        r.setflags(write=False)
        _CACHE[k] = r
    return _CACHE[k]


def restated(ref, oracle, key, scene, w, h, rows=None, ray_dir=REF_DIR):
    """(cached_hits, ref(oracle, scene, hits, row_begin, ray_dir)), once per
    restatement `ref`, key, direction and light set: the CPU and the GPU file
    of one pass share it."""
    k = (ref.__name__, key, w, h, rows, np.asarray(ray_dir, F32).tobytes(),
         np.asarray(scene.lights, F32).tobytes())
    if k not in _CACHE:
        hits = cached_hits(oracle, key, scene, w, h, rows, ray_dir)
        _CACHE[k] = (hits, ref(oracle, scene, hits, rows[0] if rows else 0, ray_dir))
    return _CACHE[k]


def _unit(mx, my, mz):
    length = np.sqrt((mx * mx + my * my) + mz * mz)
    return mx / length, my / length, mz / length


def hit_points(hits, row_begin, ray_dir, x_begin=0):
    """p = (x + t*d.x, y + t*d.y, 0 + t*d.z) per pixel, three (rows x w) arrays.
    `x_begin`: the frame column of hits[:, 0]."""
    n, w = hits.shape
    d = np.asarray(ray_dir, F32)
    x = np.broadcast_to((x_begin + np.arange(w)).astype(F32)[None, :], (n, w))
    y = np.broadcast_to((row_begin + np.arange(n)).astype(F32)[:, None], (n, w))
    t = hits["t"]
    with np.errstate(all="ignore"):
        return x + t * d[0], y + t * d[1], F32(0.0) + t * d[2]


def surfaces_ref(oracle, scene, hits, row_begin=0, ray_dir=REF_DIR, x_begin=0, flipped=None):
    """(rows x w) surface records of a hit frame band starting at row_begin
    (and at column x_begin of its frame).  `flipped`: a (rows x w) bool array
    that receives where the facing step negated the normal."""
    n, w = hits.shape
    d = np.ascontiguousarray(ray_dir, F32)
    t, obj = hits["t"], hits["object"]
    nc = scene.num_cubes
    nx, ny, nz = (np.zeros((n, w), F32) for _ in range(3))
    tri = np.full((n, w), -1, np.int32)
    px, py, pz = hit_points(hits, row_begin, d, x_begin)
    cubes = np.ascontiguousarray(scene.cube_vertices, F32).reshape(-1, 36, 4)
    with np.errstate(all="ignore"):
        for c in np.unique(obj[(obj >= 0) & (obj < nc)]):
            todo = obj == c
            for k in range(12):
                v0, v1, v2 = cubes[c, 3 * k, :3], cubes[c, 3 * k + 1, :3], cubes[c, 3 * k + 2, :3]
                td = oracle.tri_t_grid(cubes[c, 3 * k], cubes[c, 3 * k + 1], cubes[c, 3 * k + 2],
                                       d, x_begin, row_begin, w, n)
                match = todo & ~np.isnan(td) & (td.astype(F32) == t)
                if not match.any():
                    continue
                e1, e2 = v1 - v0, v2 - v0
                ux, uy, uz = _unit(e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                                   e1[0] * e2[1] - e1[1] * e2[0])
                nx[match], ny[match], nz[match], tri[match] = ux, uy, uz, k
                todo = todo & ~match
        sph = obj >= nc
        if sph.any():
            centre = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)[obj[sph] - nc]
            nx[sph], ny[sph], nz[sph] = _unit(px[sph] - centre[:, 0], py[sph] - centre[:, 1],
                                              pz[sph] - centre[:, 2])
        s = (nx * d[0] + ny * d[1]) + nz * d[2]
        flip = s > 0
        nx[flip], ny[flip], nz[flip] = -nx[flip], -ny[flip], -nz[flip]
        if flipped is not None:
            flipped[...] = flip
    out = np.empty((n, w), surface_dtype())
    out["nx"], out["ny"], out["nz"], out["triangle"] = nx, ny, nz, tri
    return out


def light_factor_ref(scene, hits, surf, row_begin=0, ray_dir=REF_DIR, x_begin=0, terms=None):
    """k per pixel: 1 without lights or without an object, else the clamped
    sum of the positive cosines.  `terms`: a dict that receives "ll" and "c"
    (lights x rows x w) and "sum" (the sum before the clamp)."""
    n, w = hits.shape
    lights = np.ascontiguousarray(scene.lights, F32).reshape(-1, 4)
    k = np.ones((n, w), F32)
    if len(lights) == 0:
        return k
    px, py, pz = hit_points(hits, row_begin, ray_dir, x_begin)
    lls, cs = [], []
    acc = np.zeros((n, w), F32)
    with np.errstate(all="ignore"):
        for l in lights:
            lx, ly, lz = l[0] - px, l[1] - py, l[2] - pz
            ll = np.sqrt((lx * lx + ly * ly) + lz * lz)
            c = ((surf["nx"] * lx + surf["ny"] * ly) + surf["nz"] * lz) / ll
            acc = np.where(c > 0, acc + c, acc)
            if terms is not None:
                lls.append(ll)
                cs.append(c)
        if terms is not None:
            terms.update(ll=np.array(lls), c=np.array(cs), sum=acc)
        acc = np.where(acc > 1, F32(1.0), acc)
    return np.where(hits["object"] == -1, F32(1.0), acc).astype(F32)


def x86_int(v):
    """(int)v as cvttss2si: NaN and out-of-range values give INT32_MIN."""
    with np.errstate(invalid="ignore"):
        ok = (v >= F32(-2147483648.0)) & (v < F32(2147483648.0))
        return np.where(ok, np.where(ok, v, F32(0.0)).astype(np.int64), INT_MIN).astype(np.int32)


def lit_ref(oracle, scene, hits, row_begin=0, ray_dir=REF_DIR, surf=None, x_begin=0, k=None):
    """The int32x4 frame of rt_light_hits (pack with oracle.pack_rgba8).
    `k`: light_factor_ref's result where the caller already has it."""
    if surf is None:
        surf = surfaces_ref(oracle, scene, hits, row_begin, ray_dir, x_begin)
    if k is None:
        k = light_factor_ref(scene, hits, surf, row_begin, ray_dir, x_begin)
    t, obj = hits["t"], hits["object"]
    table = np.concatenate([np.ascontiguousarray(scene.cube_colours, F32).reshape(-1, 4),
                            np.ascontiguousarray(scene.sphere_colours, F32).reshape(-1, 4),
                            np.array([[0, 0, 0, 255]], F32)])  # [-1]: no object
    colour = table[obj]
    out = np.zeros(hits.shape + (4,), np.int32)
    out[..., 3] = 255
    with np.errstate(all="ignore"):
        normalised = (t - F32(0.0)) / (F32(180.0) - F32(0.0))
        scalar = F32(255.0) - (normalised * F32(255.0))
        lit = scalar * k
        for ch in range(3):
            out[..., ch] = x86_int(lit * colour[..., ch])
    out[t == K_FAR] = (0, 0, 0, 255)
    return out


def words(a):
    """Any 4-byte-element array or record array as raw uint32 words."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.shape + (-1,)) if a.dtype.names else a.view(np.uint32)


def eq(got, want):
    """'' or a description of the first differing pixel (raw words)."""
    a, b = words(got), words(want)
    if a.shape != b.shape:
        return f"shape {a.shape} vs {b.shape}"
    bad = (a != b).reshape(got.shape[:2] + (-1,)).any(-1)
    if not bad.any():
        return ""
    ys, xs = np.nonzero(bad)
    return (f"{int(bad.sum())} pixels differ, first at (x={xs[0]}, y={ys[0]}): "
            f"{got[ys[0], xs[0]]} vs {want[ys[0], xs[0]]}")
