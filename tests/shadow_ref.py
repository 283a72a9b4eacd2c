"""The shadow term of the light pass -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of DESIGN.md §3.1b for rt_shadow_hits /
rt_light_hits_shadowed.  The two occluder tests are restated operation by
operation: the triangle test in `float64` arrays (the reference's
Moeller-Trumbore text on p and the un-normalised L), the sphere test in
`float32` arrays, one ufunc per written operation (numpy never contracts), in
the written order.  Surfaces, the cosines c and the final shade come from
tests/light_ref.py; hit frames from the oracle through `light_ref.cached_hits`.
"""
import numpy as np

import light_ref as lr
from gpu_support import F32
from hit_ref import REF_DIR

F64 = np.float64
EPSILON = F64(0.000001)
# the scene of the four occluder / receiver kinds (tests 1 and 4), 128 x 128
KINDS_W = KINDS_H = 128
KINDS_LIGHT = (154, 64, 40, 1)


def kinds_scene(pkg, lights=(KINDS_LIGHT,)):
    """Cube 0: a face at z = -50 that fills the frame.  Cube 1: the box
    x in [85, 97], y in [58, 70], z in [-15, -3].  Sphere 0: (64, 64, -30),
    r = 12.  Sphere 1: (118, 64, 12), r = 4, in front of the ray origins: no
    primary ray hits it, it only occludes."""
    cubes = np.array([pkg.cube_packed([("scale", 70, 70, 10), ("translate", 64, 64, -60)]),
                      pkg.cube_packed([("scale", 6, 6, 6), ("translate", 91, 64, -9)])], F32)
    return pkg.Scene(np.array([[64, 64, -30, 1], [118, 64, 12, 1]], F32), np.array([12, 4], F32),
                     np.array([[0.2, 0.9, 0.4, 255], [0.9, 0.9, 0.1, 255]], F32), cubes,
                     np.array([[1.0, 0.7, 0.3, 255], [0.3, 0.5, 1.0, 255]], F32),
                     np.array(lights, F32).reshape(-1, 4))


def wave_scene(pkg):
    """Cube 0 of kinds_scene, and one sphere at (32, 64, 20), r = 15, unseen,
    under a light at (32, 64, 60): its shadow on the face is a disc of radius
    about 44.5 about (32, 64)."""
    face = pkg.cube_packed([("scale", 70, 70, 10), ("translate", 64, 64, -60)]).reshape(1, 36, 4)
    return pkg.Scene(np.array([[32, 64, 20, 1]], F32), np.array([15], F32),
                     np.array([[0.2, 0.9, 0.4, 255]], F32), face,
                     np.array([[1.0, 0.7, 0.3, 255]], F32), np.array([[32, 64, 60, 1]], F32))


def intersecting_spheres(pkg, lights):
    """Sphere 0: (32, 24, 10), r = 30: its centre is in front of the ray
    origins, so no primary ray hits it, and it reaches back to z = -20.
    Sphere 1: (32, 24, -25), r = 10: the hit points of its front lie inside
    sphere 0."""
    return pkg.Scene(np.array([[32, 24, 10, 1], [32, 24, -25, 1]], F32), np.array([30, 10], F32),
                     np.array([[0.9, 0.2, 0.2, 255], [0.2, 0.9, 0.9, 255]], F32),
                     lights=np.array(lights, F32).reshape(-1, 4))


def lone_pixel_scene(pkg):
    """The base scene with sphere 0 moved onto pixel (0, 0), nearer than
    everything else, and sphere 1 between its hit point and the light."""
    scene = lr.with_lights(lr.base(pkg), lr.ONE_LIGHT)
    scene.sphere_origins[0] = (0, 0, -5, 1)
    scene.sphere_radius[0] = 3
    scene.sphere_origins[1] = (24, 20, 99, 1)  # half way from (0, 0, -2) to (48, 40, 200)
    scene.sphere_radius[1] = 5
    return scene


DENORMAL = float(np.float32(1e-42))
# name: lights of kinds_scene, 128 x 128 (tests 5 of the CPU file, 7 of the GPU file)
EDGE_LIGHTS = {
    # L = 0 at pixel (40, 40), whose hit point is (40, 40, -50): ll = 0, c = 0 / 0
    "light_on_a_hit_point": [(40, 40, -50, 1), KINDS_LIGHT],
    # 1e20: a and ll are infinite; 1e19: a is finite and disc = inf - inf
    "light_at_1e20": [(1e20, 64, 40, 1), (64, 1e20, 1e20, 1), (1e19, 64, 1e19, 1)],
    "light_at_inf": [(np.inf, 64, 40, 1), (64, 64, np.inf, 1), (-np.inf, 64, 40, 1)],
    "light_at_nan": [(np.nan, 64, 40, 1), KINDS_LIGHT, (154, np.nan, 40, 1)],
    "light_at_denormals": [(DENORMAL, -DENORMAL, DENORMAL, 1), KINDS_LIGHT],
    # the centre of sphere 0: every segment from outside ends inside it
    "light_inside_a_sphere": [(64, 64, -30, 1)],
    # on the back face z = -15 of cube 1: segments from behind end on it, t = 1
    "light_on_a_triangle": [(91, 64, -15, 1)],
}


def edge_cases(pkg):
    """(name, scene, w, h, ray_dir) of the shadow term's numeric edges."""
    cases = [(name, kinds_scene(pkg, lights), KINDS_W, KINDS_H, REF_DIR)
             for name, lights in EDGE_LIGHTS.items()]
    # p inside another sphere; the first light is outside that sphere, the second inside
    cases.append(("p_inside_a_sphere",
                  intersecting_spheres(pkg, [(32, 24, 100, 1), (32, 24, 0, 1)]), 64, 48, REF_DIR))
    for key, scene, w, h, d in lr.edge_scenes(pkg):
        if key in ("minus_inf", "nan_colour"):
            cases.append((key, lr.with_lights(scene, lr.THREE_LIGHTS), w, h, d))
    return cases


def tri_occludes(p, L, v0, v1, v2):
    """The test's verdict with 0 < t < 1.  A bool array."""
    hit, td = tri_td(p, L, v0, v1, v2)
    with np.errstate(all="ignore"):
        return hit & (td > 0.0) & (td < 1.0)


def tri_td(p, L, v0, v1, v2):
    """MainState.cpp:257-298 on doubles.  p, L: three float32 arrays each;
    v0..v2: float32[3].  (where the test returns 1, its t)."""
    o = [a.astype(F64) for a in p]
    d = [a.astype(F64) for a in L]
    v0, v1, v2 = (np.asarray(v, F32)[:3].astype(F64) for v in (v0, v1, v2))
    with np.errstate(all="ignore"):
        e1 = [v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]]
        e2 = [v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]]
        pv = [d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2],
              d[0] * e2[1] - d[1] * e2[0]]
        det = (e1[0] * pv[0] + e1[1] * pv[1]) + e1[2] * pv[2]
        out = ~((det > -EPSILON) & (det < EPSILON))
        inv_det = F64(1.0) / det
        tv = [o[0] - v0[0], o[1] - v0[1], o[2] - v0[2]]
        u = ((tv[0] * pv[0] + tv[1] * pv[1]) + tv[2] * pv[2]) * inv_det
        out &= ~((u < 0.0) | (u > 1.0))
        qv = [tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2],
              tv[0] * e1[1] - tv[1] * e1[0]]
        v = ((d[0] * qv[0] + d[1] * qv[1]) + d[2] * qv[2]) * inv_det
        out &= ~((v < 0.0) | (u + v > 1.0))
        td = ((e2[0] * qv[0] + e2[1] * qv[1]) + e2[2] * qv[2]) * inv_det
        return out, td


def sphere_occludes(p, L, centre, r):
    """All float32.  A bool array."""
    c, r = np.asarray(centre, F32), F32(r)
    with np.errstate(all="ignore"):
        mx, my, mz = c[0] - p[0], c[1] - p[1], c[2] - p[2]
        a = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]
        b = (mx * L[0] + my * L[1]) + mz * L[2]
        q = ((mx * mx + my * my) + mz * mz) - r * r
        disc = b * b - a * q
        sq = np.sqrt(disc)
        s0 = (b - sq) / a
        s1 = (b + sq) / a
        return (disc >= 0) & (((s0 > 0) & (s0 < 1)) | ((s1 > 0) & (s1 < 1)))


class Shadowed:
    """mask: uint32 (rows x w), bit i for light i < 32.  cast / occluded /
    by_cube / by_sphere: bool (lights x rows x w).  c: the cosines.  k: the
    shadowed factor.  lit: the int32x4 frame.  surf: the surfaces."""


def shadow_ref(oracle, scene, hits, row_begin=0, ray_dir=REF_DIR):
    n, w = hits.shape
    lights = np.ascontiguousarray(scene.lights, F32).reshape(-1, 4)
    r = Shadowed()
    r.surf = lr.surfaces_ref(oracle, scene, hits, row_begin, ray_dir)
    r.mask = np.zeros((n, w), np.uint32)
    shape = (len(lights), n, w)
    r.cast, r.occluded, r.by_cube, r.by_sphere = (np.zeros(shape, bool) for _ in range(4))
    r.c = np.zeros(shape, F32)
    r.k = np.ones((n, w), F32)
    if len(lights):
        terms = {}
        lr.light_factor_ref(scene, hits, r.surf, row_begin, ray_dir, terms=terms)
        r.c = terms["c"]
        obj = hits["object"]
        nc = scene.num_cubes
        p = lr.hit_points(hits, row_begin, ray_dir)
        cubes = np.ascontiguousarray(scene.cube_vertices, F32).reshape(-1, 36, 4)
        centres = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)
        radius = np.ascontiguousarray(scene.sphere_radius, F32).reshape(-1)
        acc = np.zeros((n, w), F32)
        with np.errstate(all="ignore"):
            for i, l in enumerate(lights):
                L = (l[0] - p[0], l[1] - p[1], l[2] - p[2])
                cast = (obj >= 0) & (r.c[i] > 0)
                r.cast[i] = cast
                for j in range(nc):
                    cand = cast & (obj != j)
                    if not cand.any():
                        continue
                    for k in range(12):
                        r.by_cube[i] |= cand & tri_occludes(p, L, *cubes[j, 3 * k:3 * k + 3])
                for s in range(len(radius)):
                    cand = cast & (obj != nc + s)
                    if cand.any():
                        r.by_sphere[i] |= cand & sphere_occludes(p, L, centres[s], radius[s])
                r.occluded[i] = r.by_cube[i] | r.by_sphere[i]
                if i < 32:
                    r.mask |= r.occluded[i].astype(np.uint32) << np.uint32(i)
                acc = np.where(cast & ~r.occluded[i], acc + r.c[i], acc)
            acc = np.where(acc > 1, F32(1.0), acc)
        r.k = np.where(obj == -1, F32(1.0), acc).astype(F32)
    r.lit = lr.lit_ref(oracle, scene, hits, row_begin, ray_dir, surf=r.surf, k=r.k)
    return r


def segments(flags):
    """Of the 64-pixel row segments of a bool frame (one per wave where the
    width is a multiple of 64): how many are wholly set, wholly clear, mixed."""
    s = flags.reshape(-1, 64)
    return int(s.all(1).sum()), int((~s.any(1)).sum()), int((s.any(1) & ~s.all(1)).sum())
