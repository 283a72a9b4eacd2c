"""The mirror bounce of the light pass -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of DESIGN.md §3.1c for rt_reflect_hits /
rt_light_hits_reflected, one ufunc per written operation (numpy never
contracts), in the written order.  The triangle test is `shadow_ref.tri_td`
(the reference's Moeller-Trumbore text in `float64` arrays, on p and the
un-normalised R); the sphere quadratic is restated here in `float32` arrays.
Surfaces, the factor k, hit points and the x86 (int) come from
tests/light_ref.py; hit frames from the oracle through `light_ref.cached_hits`.
"""
import numpy as np

import light_edges as le
import light_ref as lr
import shadow_ref as sr
from gpu_support import F32, H, W
from hit_ref import K_FAR, REF_DIR, hit_dtype

MIRROR_W = MIRROR_H = 128
OBLIQUE_DIR = (0.3, -0.2, -1.0, -1.0)


# ---------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------
def plus(pkg, scene, spheres=(), cubes=()):
    """`scene` (lights kept) plus (origin4, radius, colour4) spheres and
    (ops, colour4) cubes, last in their order."""
    so = np.array([x[0] for x in spheres], F32).reshape(-1, 4)
    rad = np.array([x[1] for x in spheres], F32).reshape(-1)
    sc = np.array([x[2] for x in spheres], F32).reshape(-1, 4)
    cv = np.array([pkg.cube_packed(c[0]) for c in cubes], F32).reshape(-1, 36, 4)
    cc = np.array([c[1] for c in cubes], F32).reshape(-1, 4)
    return pkg.Scene(np.concatenate([scene.sphere_origins, so]),
                     np.concatenate([scene.sphere_radius, rad]),
                     np.concatenate([scene.sphere_colours, sc]),
                     np.concatenate([scene.cube_vertices, cv]),
                     np.concatenate([scene.cube_colours, cc]), scene.lights)


def mirror_scene(pkg, lights=(sr.KINDS_LIGHT,)):
    """shadow_ref.kinds_scene (cube 0: the face at z = -50; cube 1: the box;
    sphere 0: (64, 64, -30), r = 12; sphere 1: (118, 64, 12), r = 4, in front
    of the ray origins), plus
      cube 2: a cube of half edge 10 turned by 60 degrees about y, at
              (30, 104, -22): one visible face mirrors down onto the face at
              z = -50 (cube -> cube), the other up and to the left;
      sphere 4: (-20, 104, 16), r = 14, left of the frame and in front of
              the ray origins, in the way of that second face's mirrored rays
              (cube -> sphere); no primary ray sees it;
      spheres 2, 3: (30, 26, -30) and (68, 26, -30), r = 18, side by side:
              their facing flanks mirror each other (sphere -> sphere).
    With d = (0, 0, -1) the face mirrors straight back (R = (0, 0, 1)) into
    sphere 1, which no primary ray sees (cube -> sphere), and the rims of the
    spheres mirror down onto the face (sphere -> cube)."""
    return plus(pkg, sr.kinds_scene(pkg, lights),
                spheres=[((30, 26, -30, 1), 18, (0.9, 0.3, 0.6, 255)),
                         ((68, 26, -30, 1), 18, (0.4, 0.8, 0.9, 255)),
                         ((-20, 104, 16, 1), 14, (0.8, 0.8, 0.2, 255))],
                cubes=[([("scale", 10, 10, 10), ("rotate", 0, np.pi / 3, 0),
                         ("translate", 30, 104, -22)], (0.6, 1.0, 0.5, 255))])


def ramp_scene(pkg, lights=()):
    """The face at z = -50 and one sphere at (32, 24, 100), r = 10, far in
    front of the ray origins: the face mirrors it at best of about 140 to 150,
    so t + best is past the ramp's end at 180."""
    face = pkg.cube_packed(_FACE).reshape(1, 36, 4)
    return pkg.Scene(np.array([[32, 24, 100, 1]], F32), np.array([10], F32),
                     np.array([[0.9, 0.8, 0.7, 255]], F32), face,
                     np.array([[1.0, 0.7, 0.3, 255]], F32), np.array(lights, F32).reshape(-1, 4))


_FACE = [("scale", 70, 70, 10), ("translate", 32, 24, -60)]  # its near side: z = -50
_BOX = [("scale", 5, 10, 10), ("translate", 55, 24, -35)]


def twin_cubes_scene(pkg):
    """A sphere at (32, 24, -30), r = 12, and beside it two identical boxes
    (cubes 0 and 1), x in [50, 60]: the sphere's right flank mirrors into
    them, and every candidate of cube 1 ties with cube 0's."""
    return plus(pkg, pkg.Scene(), spheres=[((32, 24, -30, 1), 12, (0.9, 0.8, 0.7, 255))],
                cubes=[(_BOX, (0.2, 0.9, 0.4, 255)), (_BOX, (0.9, 0.2, 0.9, 255))])


TIE_PIXEL = (16, 26)  # (y, x)
TIE_CENTRE = (85.37, 24, -50, 1)
TIE_RADIUS = np.uint32(0x41015666).view(F32)  # 8.083593...


def sphere_tie_scene(pkg):
    """The face at z = -50 (cube 0), a cube turned by 60 degrees about y
    (cube 1) whose visible face mirrors down and to the right onto it, and a
    sphere whose centre lies in the face's plane, right of the frame.  The
    mirrored ray of pixel TIE_PIXEL meets the face's plane on the sphere's
    rim: TIE_RADIUS was searched for (by bisection on the restatement, among
    neighbouring floats) so that the quadratic's s0 and the triangle's
    (float)td are the same float there.  The test asserts that they are."""
    tilt = [("scale", 8, 8, 8), ("rotate", 0, np.pi / 3, 0), ("translate", 20, 24, -22)]
    return plus(pkg, pkg.Scene(), spheres=[(TIE_CENTRE, TIE_RADIUS, (0.2, 0.4, 0.9, 255))],
                cubes=[(_FACE, (1.0, 0.7, 0.3, 255)), (tilt, (0.2, 0.9, 0.4, 255))])


def wave_scene(pkg, lights=()):
    """A face at z = -50 over x < 90 and y in [30, 100], and sphere 1 of
    kinds_scene moved to (40, 64, 12), unseen: at 128 x 128 the left 64-pixel
    segment of rows 30..100 is wholly hit, the right one mixed, the other rows
    wholly missed."""
    face = [("scale", 50, 35, 10), ("translate", 40, 65, -60)]
    return plus(pkg, pkg.Scene(lights=np.array(lights, F32).reshape(-1, 4)),
                spheres=[((40, 64, 12, 1), 8, (0.9, 0.9, 0.1, 255))],
                cubes=[(face, (1.0, 0.7, 0.3, 255))])


# the numeric edges both test files run (tests/test_reflect_hits.py says what each holds)
def slab_with_a_target(pkg):
    """light_edges' underflow slab (every normal NaN) and a sphere behind it."""
    return plus(pkg, le.slab(1e-30)(pkg), spheres=[((40, 32, -1e26, 1), 1e25, le.BRIGHT)])


def edge_cases(pkg):
    """name -> (scene, w, h, ray_dir, hit-cache key)."""
    cases = {name: (mirror_scene(pkg, lights), MIRROR_W, MIRROR_H, REF_DIR, "mirror")
             for name, lights in sr.EDGE_LIGHTS.items()}
    cases["dir_oblique"] = (mirror_scene(pkg), MIRROR_W, MIRROR_H, OBLIQUE_DIR,
                            "mirror")
    cases["dir_oblique_base"] = (lr.with_lights(le.base_rewound(pkg), lr.THREE_LIGHTS), W, H,
                                 (0.3, -0.2, -1, -1), "base_rewound")
    cases["dir_scaled_-1e-4"] = (lr.with_lights(le.base_near(pkg), lr.THREE_LIGHTS), W, H,
                                 (0, 0, -1e-4, -1), "base_near")
    cases["dir_scaled_-1e30"] = (lr.with_lights(lr.base(pkg), lr.THREE_LIGHTS), W, H,
                                 (0, 0, -1e30, -1), "base")
    cases["nan_normal"] = (lr.with_lights(slab_with_a_target(pkg), le.SLAB_LIGHTS), 2, 64,
                           (0, 0, -1e25, 0), "reflect_slab")
    for key, scene, w, h, d in lr.edge_scenes(pkg):
        if key in ("minus_inf", "nan_colour"):
            cases[key] = (lr.with_lights(scene, lr.THREE_LIGHTS), w, h, d, "shadow_edge_" + key)
    return cases


EDGE_NAMES = sorted(sr.EDGE_LIGHTS) + ["dir_oblique", "dir_oblique_base", "dir_scaled_-1e-4",
                                       "dir_scaled_-1e30", "nan_normal", "minus_inf",
                                       "nan_colour"]



# ---------------------------------------------------------------------------
# The restatement
# ---------------------------------------------------------------------------
def mirror_dir(surf, ray_dir):
    """R = d - (s + s) * n per pixel, three float32 arrays."""
    d = np.asarray(ray_dir, F32)
    nx, ny, nz = surf["nx"], surf["ny"], surf["nz"]
    with np.errstate(all="ignore"):
        s = (nx * d[0] + ny * d[1]) + nz * d[2]
        f = s + s
        return d[0] - f * nx, d[1] - f * ny, d[2] - f * nz


def sphere_sf(p, R, centre, r):
    """The quadratic of §3.1b on R.  (candidate, sf)."""
    c, r = np.asarray(centre, F32), F32(r)
    with np.errstate(all="ignore"):
        mx, my, mz = c[0] - p[0], c[1] - p[1], c[2] - p[2]
        a = (R[0] * R[0] + R[1] * R[1]) + R[2] * R[2]
        b = (mx * R[0] + my * R[1]) + mz * R[2]
        q = ((mx * mx + my * my) + mz * mz) - r * r
        disc = b * b - a * q
        sq = np.sqrt(disc)
        s0 = (b - sq) / a
        s1 = (b + sq) / a
        near, far = s0 > 0, s1 > 0
        return (disc >= 0) & (near | far), np.where(near, s0, s1), (disc >= 0) & ~near & far


def tri_sf(p, R, v0, v1, v2):
    """(candidate, sf = (float)td) of one triangle."""
    ok, td = sr.tri_td(p, R, v0, v1, v2)
    with np.errstate(all="ignore"):
        return ok & (td > 0.0), td.astype(F32)


def factor_at(n, p, lights):
    """light_factor (§3.1a) at the points p with the normals n: the operations
    of light_ref.light_factor_ref, which takes its points from a hit frame."""
    acc = np.zeros(p[0].shape, F32)
    with np.errstate(all="ignore"):
        for l in lights:
            lx, ly, lz = l[0] - p[0], l[1] - p[1], l[2] - p[2]
            ll = np.sqrt((lx * lx + ly * ly) + lz * lz)
            c = ((n[0] * lx + n[1] * ly) + n[2] * lz) / ll
            acc = np.where(c > 0, acc + c, acc)
        return np.where(acc > 1, F32(1.0), acc).astype(F32)


def _unit(mx, my, mz):
    with np.errstate(all="ignore"):
        length = np.sqrt((mx * mx + my * my) + mz * mz)
        return mx / length, my / length, mz / length


def walk(scene, own, p, R):
    """bounce_walk from the points p along R over every object but `own` (-1:
    no walk there): cubes 0 .. nc-1 with triangles 0 .. 11, then spheres; a
    candidate is taken iff sf < best.  (best, obj2, tri2, far_root: the
    winning sphere root was s1)."""
    cubes = np.ascontiguousarray(scene.cube_vertices, F32).reshape(-1, 36, 4)
    centres = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)
    radius = np.ascontiguousarray(scene.sphere_radius, F32).reshape(-1)
    nc = len(cubes)
    best = np.full(own.shape, K_FAR, F32)
    obj2 = np.full(own.shape, -1, np.int32)
    tri2 = np.full(own.shape, -1, np.int32)
    far_root = np.zeros(own.shape, bool)
    active = own >= 0
    with np.errstate(all="ignore"):
        for j in range(nc):
            cand = active & (own != j)
            if not cand.any():
                continue
            for k in range(12):
                ok, sf = tri_sf(p, R, *cubes[j, 3 * k:3 * k + 3])
                take = cand & ok & (sf < best)
                best, obj2, tri2 = (np.where(take, sf, best), np.where(take, j, obj2),
                                    np.where(take, k, tri2))
        for s in range(len(radius)):
            cand = active & (own != nc + s)
            if not cand.any():
                continue
            ok, sf, far = sphere_sf(p, R, centres[s], radius[s])
            take = cand & ok & (sf < best)
            best, obj2, tri2 = (np.where(take, sf, best), np.where(take, nc + s, obj2),
                                np.where(take, -1, tri2))
            far_root = np.where(take, far, far_root)
    return best.astype(F32), obj2.astype(np.int32), tri2.astype(np.int32), far_root


def normal_at(scene, obj2, tri2, p2, R):
    """bounce_normal: the unit normal of (obj2, tri2) at p2, turned against R
    (0 where obj2 is -1)."""
    cubes = np.ascontiguousarray(scene.cube_vertices, F32).reshape(-1, 36, 4)
    centres = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)
    nc = len(cubes)
    n2 = [np.zeros(obj2.shape, F32) for _ in range(3)]
    on_cube = (obj2 >= 0) & (obj2 < nc)
    with np.errstate(all="ignore"):
        for j, k in sorted({(int(a), int(b)) for a, b in zip(obj2[on_cube], tri2[on_cube])}):
            v0, v1, v2 = cubes[j, 3 * k, :3], cubes[j, 3 * k + 1, :3], cubes[j, 3 * k + 2, :3]
            e1, e2 = v1 - v0, v2 - v0
            u = _unit(e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                      e1[0] * e2[1] - e1[1] * e2[0])
            at = (obj2 == j) & (tri2 == k)
            for c in range(3):
                n2[c][at] = u[c]
        sph = obj2 >= nc
        if sph.any():
            c = centres[obj2[sph] - nc]
            u = _unit(p2[0][sph] - c[:, 0], p2[1][sph] - c[:, 1], p2[2][sph] - c[:, 2])
            for i in range(3):
                n2[i][sph] = u[i]
        s = (n2[0] * R[0] + n2[1] * R[1]) + n2[2] * R[2]
        flip = s > 0
        return [np.where(flip, -a, a) for a in n2]


def ramp(T, clamped):
    """The depth ramp at depth T; `clamped`: never below 0 (every level but
    the pixel's own: past the ramp's end a bounce adds no negative light)."""
    with np.errstate(all="ignore"):
        normalised = (T - F32(0.0)) / (F32(180.0) - F32(0.0))
        scalar = F32(255.0) - (normalised * F32(255.0))
        return np.where(scalar > 0, scalar, F32(0.0)) if clamped else scalar


def mix(a, b, r):
    """a + r * (b - a), in float32."""
    with np.errstate(all="ignore"):
        return a + r * (b - a)


def blended(lit, r, lit1, lit2, rf):
    """`lit` with (int)(a + r * (b - a)) in the colour channels where `rf`
    (a Reflected) blends: a = lit1 * the pixel's colour, b = lit2 * the
    bounce's."""
    r = F32(r)
    if r == 0:
        return lit
    out = np.array(lit)
    with np.errstate(all="ignore"):
        for ch in range(3):
            a, b = lit1 * rf._colour[..., ch], lit2 * rf._colour2[..., ch]
            out[..., ch] = np.where(rf._blend, lr.x86_int(mix(a, b, r)), out[..., ch])
    return out


class Reflected:
    """bounce: the HIT_DTYPE frame of rt_reflect_hits.  tri2: the bounce's
    triangle (-1: sphere or miss).  kinds: {(receiver, target): bool frame}
    over "cube" / "sphere".  far_root: where the winning sphere root was s1.
    R, p: the mirrored direction and the hit point.  surf, k: the primary
    surfaces and factor.  lit: rt_light_hits' int32x4 frame.  mirrored(r):
    rt_light_hits_reflected's.  scalar2: the bounce's ramp before the clamp
    (NaN where the bounce missed)."""

    def mirrored(self, r):
        return blended(self.lit, r, self._lit, self._lit2, self)


def reflect_ref(oracle, scene, hits, row_begin=0, ray_dir=REF_DIR):
    """Level 0, one walk, the normal and the factor at the bounce point."""
    n, w = hits.shape
    t, obj = hits["t"], hits["object"]
    nc = scene.num_cubes
    lights = np.ascontiguousarray(scene.lights, F32).reshape(-1, 4)
    r = Reflected()
    r.surf = lr.surfaces_ref(oracle, scene, hits, row_begin, ray_dir)
    r.k = lr.light_factor_ref(scene, hits, r.surf, row_begin, ray_dir)
    r.lit = lr.lit_ref(oracle, scene, hits, row_begin, ray_dir, surf=r.surf, k=r.k)
    r.p = p = lr.hit_points(hits, row_begin, ray_dir)
    r.R = R = mirror_dir(r.surf, ray_dir)
    best, obj2, r.tri2, r.far_root = walk(scene, obj.astype(np.int32), p, R)
    r.bounce = np.empty((n, w), hit_dtype())
    r.bounce["t"], r.bounce["object"] = best, obj2
    hit2 = obj2 >= 0
    kind = {"cube": (obj >= 0) & (obj < nc), "sphere": obj >= nc}
    kind2 = {"cube": hit2 & (obj2 < nc), "sphere": obj2 >= nc}
    r.kinds = {(a, b): kind[a] & kind2[b] for a in kind for b in kind2}

    # the mirrored pixel
    table = np.concatenate([np.ascontiguousarray(scene.cube_colours, F32).reshape(-1, 4),
                            np.ascontiguousarray(scene.sphere_colours, F32).reshape(-1, 4),
                            np.array([[0, 0, 0, 255]], F32)])  # [-1]: nothing
    r._colour, r._colour2 = table[obj], table[obj2]
    r._blend = (obj >= 0) & ~(t == K_FAR)
    with np.errstate(all="ignore"):
        r._lit = ramp(t, False) * r.k
        p2 = (p[0] + best * R[0], p[1] + best * R[1], p[2] + best * R[2])
        r.n2 = normal_at(scene, obj2, r.tri2, p2, R)
        k2 = factor_at(r.n2, p2, lights) if len(lights) else np.ones((n, w), F32)
        r.scalar2 = np.where(hit2, ramp(t + best, False), F32(np.nan))
        r._lit2 = np.where(hit2, ramp(t + best, True) * k2, F32(0.0)).astype(F32)
    r.k2 = np.where(hit2, k2, F32(np.nan))
    return r


# ---------------------------------------------------------------------------
# What the tests of both files (CPU and GPU) share
# ---------------------------------------------------------------------------
def restated(oracle, key, scene, w, h, rows=None, d=REF_DIR):
    """(hits, reflect_ref's restatement), once per key, direction and light set."""
    return lr.restated(reflect_ref, oracle, key, scene, w, h, rows, d)


def lone_pixel_scene(pkg):
    """The base scene with sphere 0 moved onto pixel (0, 0), nearer than
    everything else, and sphere 1 straight above it, in front of the ray
    origins: the pixel mirrors it."""
    scene = lr.with_lights(lr.base(pkg), lr.ONE_LIGHT)
    scene.sphere_origins[0] = (0, 0, -5, 1)
    scene.sphere_radius[0] = 3
    scene.sphere_origins[1] = (0, 0, 20, 1)
    scene.sphere_radius[1] = 5
    return scene


def check_edge(name, scene, hits, r):
    """The restatement holds what the case of edge_cases is there for."""
    obj, o2, k2 = hits["object"], r.bounce["object"], r.k2
    met = o2 >= 0
    if name in sr.EDGE_LIGHTS:
        assert met.sum() >= 1000 and not np.isnan(k2[met]).any()
    if name == "light_on_a_hit_point":
        assert (k2[met] == 0).sum() >= 20 and (k2[met] == 1).sum() >= 100
    elif name == "light_at_1e20":
        # at 1e20 ll is infinite and c = 0; the light at 1e19 alone gives 0 < k2 < 1
        assert ((k2 > 0) & (k2 < 1)).sum() >= 500 and not (k2[met] == 1).any()
    elif name == "light_at_inf":
        assert (k2[met] == 0).all()  # every c is 0 or NaN: nothing is added
    elif name == "light_at_nan":
        assert ((k2 > 0) & (k2 < 1)).sum() >= 500  # the finite light alone
    elif name == "light_at_denormals":
        assert (k2[met] == 1).sum() >= 100 and ((k2 > 0) & (k2 < 1)).sum() >= 100
    elif name in ("light_inside_a_sphere", "light_on_a_triangle"):
        assert (k2[met] == 0).sum() >= 50 and ((k2 > 0) & (k2 < 1)).sum() >= 500
    elif name in ("dir_oblique", "dir_oblique_base"):
        assert min(v.sum() for v in r.kinds.values()) >= 10
        assert (r.R[0][met] != 0).all()
    elif name == "dir_scaled_-1e-4":
        # |R| = 1e-4: parameters of thousands, far roots and a ramp long past its end
        assert met.sum() >= 500 and (r.bounce["t"][met] > 1000).sum() >= 500
        assert r.far_root.sum() >= 100 and (r.scalar2[met] < 0).sum() >= 500
    elif name in ("dir_scaled_-1e30", "nan_normal"):
        on = obj >= 0
        assert on.sum() >= 64 and np.isnan(r.surf["nx"][on]).all()
        assert all(np.isnan(c[on]).all() for c in r.R)
        assert scene.num_cubes + scene.num_spheres >= 2 and not met.any()
    elif name == "minus_inf":
        assert np.isneginf(hits["t"]).sum() > 50 and not met.any()
    elif name == "nan_colour":
        assert np.isnan(scene.sphere_colours).any() and (r.mirrored(1.0) == lr.INT_MIN).any()
    elif name not in sr.EDGE_LIGHTS:
        raise AssertionError(name)
