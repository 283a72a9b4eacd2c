"""The ray queries -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of DESIGN.md §3.1f for rt_cast_rays / rt_occlude_rays /
rt_camera_rays / rt_cast_camera.  A thin layer: the closest-hit walk is
`reflect_ref.walk`, the two occluder tests are `shadow_ref.tri_occludes` and
`sphere_occludes`, all three as they are (they take arbitrary origins,
directions and own objects already).  New here is the camera arithmetic, in
`float32` arrays with one ufunc per written operation (numpy never contracts),
in the written order, and what the tests of both files (CPU and GPU) share.
"""
import numpy as np

import light_ref as lr
import reflect_ref as rr
import shadow_ref as sr
from gpu_support import F32
from hit_ref import hit_dtype

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def ray_dtype():
    return np.dtype([("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("skip", "<i4"),
                     ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("reserved", "<f4")])


def make_rays(o, d, skip=-1):
    """A ray array from three origin and three direction arrays (or scalars)."""
    shape = np.broadcast(*o, *d, skip).shape
    rays = np.zeros(shape, ray_dtype())
    for name, a in zip(("ox", "oy", "oz", "dx", "dy", "dz"), (*o, *d)):
        rays[name] = np.asarray(a, F32)
    rays["skip"] = skip
    return rays


def origins(rays):
    return rays["ox"], rays["oy"], rays["oz"]


def directions(rays):
    return rays["dx"], rays["dy"], rays["dz"]


def slots(scene):
    return scene.num_cubes + scene.num_spheres


# ---------------------------------------------------------------------------
# The restatement
# ---------------------------------------------------------------------------
def cast(scene, rays):
    """rt_cast_rays: (HIT_DTYPE hits, int32 triangles, far_root) per ray.
    `reflect_ref.walk` reads own == -1 as "no walk there"; a ray with skip ==
    -1 walks over every object, so it is handed an id no object has."""
    skip = rays["skip"].astype(np.int32)
    own = np.where(skip < 0, np.int32(slots(scene)), skip).astype(np.int32)
    best, obj2, tri2, far = rr.walk(scene, own, origins(rays), directions(rays))
    hits = np.empty(rays.shape, hit_dtype())
    hits["t"], hits["object"] = best, obj2
    return hits, tri2, far


def occlude(scene, rays):
    """rt_occlude_rays: uint8 per ray, and what occluded it: (any, by a cube,
    by a sphere)."""
    cubes = np.ascontiguousarray(scene.cube_vertices, F32).reshape(-1, 36, 4)
    centres = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)
    radius = np.ascontiguousarray(scene.sphere_radius, F32).reshape(-1)
    p, L, skip = origins(rays), directions(rays), rays["skip"]
    by_cube, by_sphere = np.zeros(rays.shape, bool), np.zeros(rays.shape, bool)
    for j in range(len(cubes)):
        for k in range(12):
            by_cube |= (skip != j) & sr.tri_occludes(p, L, *cubes[j, 3 * k:3 * k + 3])
    for s in range(len(radius)):
        by_sphere |= (skip != len(cubes) + s) & sr.sphere_occludes(p, L, centres[s], radius[s])
    return (by_cube | by_sphere).astype(np.uint8), by_cube, by_sphere


def camera(cam, width, rows):
    """rt_camera_rays: rows [rows[0], rows[1]) of `cam`'s frame, row-major."""
    rb, re = rows
    fx = np.broadcast_to(np.arange(width).astype(F32)[None, :], (re - rb, width))
    fy = np.broadcast_to(np.arange(rb, re).astype(F32)[:, None], (re - rb, width))
    v = {n: np.asarray(getattr(cam, n), F32) for n in ("o0", "ou", "ov", "d0", "du", "dv")}
    with np.errstate(all="ignore"):
        o = [(v["o0"][a] + fx * v["ou"][a]) + fy * v["ov"][a] for a in range(3)]
        d = [(v["d0"][a] + fx * v["du"][a]) + fy * v["dv"][a] for a in range(3)]
        if cam.normalise:
            length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            d = [d[0] / length, d[1] / length, d[2] / length]
    return make_rays(o, d, -1)


# ---------------------------------------------------------------------------
# What the tests of both files share
# ---------------------------------------------------------------------------
def bounce_rays(hits, r):
    """The hit pixels of a reflect_ref restatement `r` as rays, in pixel
    order: (p, R, skip = the pixel's object), and where they are."""
    on = hits["object"] >= 0
    return make_rays([a[on] for a in r.p], [a[on] for a in r.R], hits["object"][on]), on


def facing_segments(oracle, scene, hits, light):
    """The segments of the shadow term for light number `light`: (rays, where):
    the hit pixels it faces (c > 0, from light_ref's surfaces and cosines) as
    (p, L = light - p, skip = the pixel's object)."""
    surf = lr.surfaces_ref(oracle, scene, hits)
    terms = {}
    lr.light_factor_ref(scene, hits, surf, terms=terms)
    where = (hits["object"] >= 0) & (terms["c"][light] > 0)
    p = lr.hit_points(hits, 0, (0.0, 0.0, -1.0, -1.0))
    l = np.asarray(scene.lights, F32).reshape(-1, 4)[light]
    with np.errstate(all="ignore"):
        L = [l[a] - p[a] for a in range(3)]
    return make_rays([a[where] for a in p], [a[where] for a in L], hits["object"][where]), where


def random_rays(scene, n, seed, box=((-20, 120), (-20, 100), (-120, 60)), skips=None):
    """`n` seeded rays: origins in `box`, directions of length 0.5 .. 200
    towards a point of the box, skip from `skips` (default: -1 and every slot)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(box, np.float64).T
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.uniform(lo, hi, (n, 3)) - o
    d *= (rng.uniform(0.5, 200.0, n) / np.linalg.norm(d, axis=1))[:, None]
    if skips is None:
        skips = np.arange(-1, slots(scene))
    skip = rng.choice(np.asarray(skips), n)
    return make_rays(o.T.astype(F32), d.T.astype(F32), skip.astype(np.int32))


def generic_camera(normalise):
    """Every vector of the camera in use, no component zero."""
    return dict(o0=(3.5, -2.25, 40.0), ou=(1.0, 0.125, -0.5), ov=(-0.25, 1.0, 0.0625),
                d0=(-0.4, -0.3, -1.0), du=(0.02, 0.001, 0.0005), dv=(-0.0015, 0.02, 0.001),
                normalise=normalise)


# name -> rays of the numeric edges, built on the base scene `scene`; the tests
# say what each holds (check_edge)
def edge_rays(scene):
    nan, inf = np.nan, np.inf
    centre, radius = scene.sphere_origins[0], float(scene.sphere_radius[0])
    base = random_rays(scene, 256, 5, skips=[-1])
    cases = {}
    for name, values in (("nan", (nan,)), ("inf", (inf, -inf))):
        rays = np.tile(base[:96], len(values))
        for v, value in enumerate(values):
            for f, field in enumerate(("ox", "oy", "oz", "dx", "dy", "dz")):
                sel = slice(96 * v + 16 * f, 96 * v + 16 * f + 12)  # 4 of 16 stay finite
                rays[field][sel] = value
        cases[name] = rays
    zero = base.copy()
    for field in ("dx", "dy", "dz"):
        zero[field][::2] = 0.0
    zero["dz"][::4] = -0.0
    # every other zero ray starts inside sphere 0
    zero["ox"][::4], zero["oy"][::4], zero["oz"][::4] = centre[0], centre[1], centre[2]
    cases["zero_direction"] = zero
    for name, length in (("length_1e-4", 1e-4), ("length_1e30", 1e30)):
        rays = random_rays(scene, 1024, 6, skips=[-1])
        with np.errstate(all="ignore"):
            norm = np.sqrt(rays["dx"].astype(np.float64) ** 2 + rays["dy"].astype(np.float64) ** 2 +
                           rays["dz"].astype(np.float64) ** 2)
            for field in ("dx", "dy", "dz"):
                rays[field] = (rays[field] / norm * length).astype(F32)
        cases[name] = rays
    rng = np.random.default_rng(8)
    n = 128
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    inside = centre[:3] + u * rng.uniform(0, 0.9 * radius, n)[:, None]
    v = rng.normal(size=(n, 3))
    v *= (rng.uniform(0.5, 3.0 * radius, n) / np.linalg.norm(v, axis=1))[:, None]
    cases["inside_a_sphere"] = make_rays(inside.T.astype(F32), v.T.astype(F32), -1)
    # on a triangle, exactly: the first vertex of every triangle of cubes 0 .. 3
    # (a point inside a face is not a float triple), towards the cube's centre
    # and past it, and away from it
    on = scene.cube_vertices[:4, ::3, :3].reshape(-1, 3).astype(np.float64)
    mid = np.repeat(scene.cube_vertices[:4, :, :3].astype(np.float64).mean(1), 12, 0)
    w = (mid - on) * np.where(np.arange(len(on)) % 3 == 2, -1.0, 4.0)[:, None]
    cases["on_a_triangle"] = make_rays(on.T.astype(F32), w.T.astype(F32), -1)
    # one set of rays through the scene, once per object left out (and once with none)
    through = random_rays(scene, 24, 9, skips=[-1])
    each = np.tile(through, slots(scene) + 1)
    each["skip"] = np.repeat(np.arange(-1, slots(scene)), len(through))
    cases["skip_each_object"] = each
    return cases


EDGE_NAMES = ["nan", "inf", "zero_direction", "length_1e-4", "length_1e30", "inside_a_sphere",
              "on_a_triangle", "skip_each_object"]


def check_edge(name, scene, rays, hits, far, occluded):
    """The restatement holds what the case is there for."""
    t, obj = hits["t"], hits["object"]
    assert not np.isnan(t).any() and (t <= 300000.0).all(), name  # no created NaN in a word
    fields = np.stack([rays[f] for f in ("ox", "oy", "oz", "dx", "dy", "dz")])
    if name in ("nan", "inf"):
        odd = ~np.isfinite(fields).all(0)
        assert all((np.isnan if name == "nan" else np.isinf)(f).sum() >= 12 for f in fields)
        assert odd.sum() >= 72 and (~odd).sum() >= 20
        assert (obj[odd] == -1).all() and not occluded[odd].any()  # no candidate, not occluded
        assert (obj[~odd] >= 0).sum() >= 5
        if name == "inf":
            assert (fields == -np.inf).any() and (fields == np.inf).any()
    elif name == "zero_direction":
        still = (fields[3:] == 0).all(0)
        assert still.sum() == 128 and np.signbit(rays["dz"][still]).sum() >= 32
        assert (obj[still] == -1).all() and not occluded[still].any()
        assert (obj[~still] >= 0).sum() >= 20
    elif name == "length_1e-4":
        # parameters in units of 1e-4: thousands, and past 300000 a miss
        assert (obj >= 0).sum() >= 50 and (t[obj >= 0] > 1000).all()
        assert occluded.sum() == 0  # nothing lies within 1e-4 of an origin
    elif name == "length_1e30":
        # a = |d|^2 overflows: no sphere is ever a candidate; the fp64 triangles are
        nc = scene.num_cubes
        assert ((obj >= 0) & (obj < nc)).sum() >= 20 and not (obj >= nc).any()
        assert (t[obj >= 0] < 1e-25).all() and occluded.sum() >= 20
    elif name == "inside_a_sphere":
        assert (far & (obj == scene.num_cubes)).sum() >= 64  # the far root of sphere 0
    elif name == "on_a_triangle":
        # ray i starts on vertex 0 of triangle i % 12 of cube i // 12: td == 0.0 there,
        # which is no candidate (td > 0) and no occluder (0 < td)
        own, touched = np.arange(len(rays)) // 12, np.zeros(len(rays), bool)
        for i in range(len(rays)):
            one = rays[i:i + 1]
            v = scene.cube_vertices[own[i], 3 * (i % 12):3 * (i % 12) + 3]
            ok, td = sr.tri_td(origins(one), directions(one), *v)
            touched[i] = ok[0] and td[0] == 0.0
        assert len(rays) == 48 and touched.sum() >= 40
        # through the cube's centre: out of the opposite corner, at 2 / 4 of 4 * (mid - on)
        into = np.arange(len(rays)) % 3 != 2
        assert (touched & into & (obj == own) & (t >= 0.25)).sum() >= 10
        assert (touched & ~into & (obj != own)).sum() >= 5
    elif name == "skip_each_object":
        n = slots(scene)
        per = len(rays) // (n + 1)
        skip = rays["skip"]
        assert set(np.unique(skip)) == set(range(-1, n))
        assert not ((obj == skip) & (skip >= 0)).any()
        free = obj[:per]
        changed = [s for s in range(n)
                   if (obj[(s + 1) * per:(s + 2) * per] != free).any()]
        assert len(changed) >= 5 and set(changed) == set(free[free >= 0])
    else:
        raise AssertionError(name)
