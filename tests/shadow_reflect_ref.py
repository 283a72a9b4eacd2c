"""Shadows and the mirror bounce together -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of DESIGN.md §3.1d for rt_shadow_hits_reflected /
rt_light_hits_shadowed_reflected.  `shadow_at` restates shadow_mask and
shadowed_factor (§3.1b) at arbitrary points, with the occluder tests of
tests/shadow_ref.py (`tri_occludes`, `sphere_occludes`); the combined frame and
the mask at p2 are built from what tests/reflect_ref.py's `reflect_ref` gives:
p, R, the bounce, tri2 and n2.  One ufunc per written operation (numpy never
contracts), in the written order.
"""
import numpy as np

import light_ref as lr
import reflect_ref as rr
import shadow_ref as sr
from gpu_support import F32
from hit_ref import REF_DIR

CLASS_W = CLASS_H = 128
# a second light, left of the frame and low: it faces what KINDS_LIGHT does not
LOW_LIGHT = (-40, 20, -20, 1)
CLASS_LIGHTS = (sr.KINDS_LIGHT, LOW_LIGHT)


# ---------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------
def class_scene(pkg, lights=CLASS_LIGHTS):
    """reflect_ref.mirror_scene under two lights, plus
      sphere 5: (100, 104, -34), r = 10, hovering 6 above the face at z = -50:
              its flanks mirror down onto the face around it, into its own
              shadow (the primary pixel's own object hides the light at p2).
    tests/test_shadow_reflect_hits.py proves on the restatement what the frame
    holds."""
    return rr.plus(pkg, rr.mirror_scene(pkg, lights),
                   spheres=[((100, 104, -34, 1), 10, (0.7, 0.4, 0.9, 255))])


WAVE_LIGHTS = {"above": [(32, 50, 200, 1)], "beside": [(150, 50, 60, 1)]}


def wave_scene(pkg, lights=WAVE_LIGHTS["above"]):
    """reflect_ref.wave_scene's face (cube 0: z = -50 over x < 90 and y in
    [30, 100]) under one sphere at (32, 50, 60), r = 40, in front of the ray
    origins and unseen.  The face mirrors straight back into its underside:
    at 128 x 128 the left 64-pixel segments of rows 30..73 are waves whose
    bounces all hit, those of rows 91..100 waves whose bounces all miss, the
    rows between and the right segments hold mixed bounces.  Under the light
    "above" the sphere no point of its underside faces the light; the light
    "beside" it, at its centre's height, faces the right half of the underside
    only."""
    face = [("scale", 50, 35, 10), ("translate", 40, 65, -60)]
    return rr.plus(pkg, pkg.Scene(lights=np.array(lights, F32).reshape(-1, 4)),
                   spheres=[((32, 50, 60, 1), 40, (0.9, 0.9, 0.1, 255))],
                   cubes=[(face, (1.0, 0.7, 0.3, 255))])


def single_object_scene(pkg):
    """A single object casts no shadow and mirrors nothing: one sphere."""
    return lr.with_lights(lr.one_sphere(pkg, (32, 24, -50, 1), 20, (1.0, 0.5, 0.25, 255)),
                          lr.THREE_LIGHTS)


# ---------------------------------------------------------------------------
# The restatement
# ---------------------------------------------------------------------------
class At:
    """shadow_at's result.  c: the cosines (lights x rows x w).  cast: the
    point is active and c > 0.  by_object: (lights x slots x rows x w), cast
    and that slot cuts the segment.  by_cube / by_sphere / occluded: their
    unions.  mask: uint32, bit i for light i < 32.  k: the shadowed factor (1
    where the point is not active, and without lights)."""


def shadow_at(scene, own, n, p):
    """shadow_mask and shadowed_factor (§3.1b) at the points `p` (three float32
    arrays) with the faced normals `n` (three float32 arrays) and the own
    object `own` per point (int32; -1: no point there)."""
    shape = own.shape
    lights = np.ascontiguousarray(scene.lights, F32).reshape(-1, 4)
    cubes = np.ascontiguousarray(scene.cube_vertices, F32).reshape(-1, 36, 4)
    centres = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)
    radius = np.ascontiguousarray(scene.sphere_radius, F32).reshape(-1)
    nc, slots = len(cubes), len(cubes) + len(radius)
    r = At()
    r.c = np.zeros((len(lights),) + shape, F32)
    r.cast = np.zeros((len(lights),) + shape, bool)
    r.by_object = np.zeros((len(lights), slots) + shape, bool)
    r.mask = np.zeros(shape, np.uint32)
    r.k = np.ones(shape, F32)
    active = own >= 0
    acc = np.zeros(shape, F32)
    with np.errstate(all="ignore"):
        for i, l in enumerate(lights):
            L = (l[0] - p[0], l[1] - p[1], l[2] - p[2])
            ll = np.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
            r.c[i] = ((n[0] * L[0] + n[1] * L[1]) + n[2] * L[2]) / ll
            cast = r.cast[i] = active & (r.c[i] > 0)
            for j in range(nc):
                cand = cast & (own != j)
                if not cand.any():
                    continue
                for k in range(12):
                    r.by_object[i, j] |= cand & sr.tri_occludes(p, L, *cubes[j, 3 * k:3 * k + 3])
            for s in range(len(radius)):
                cand = cast & (own != nc + s)
                if cand.any():
                    r.by_object[i, nc + s] = cand & sr.sphere_occludes(p, L, centres[s], radius[s])
        r.by_cube = r.by_object[:, :nc].any(1)
        r.by_sphere = r.by_object[:, nc:].any(1)
        r.occluded = r.by_cube | r.by_sphere
        for i in range(len(lights)):
            if i < 32:
                r.mask |= r.occluded[i].astype(np.uint32) << np.uint32(i)
            acc = np.where(r.cast[i] & ~r.occluded[i], acc + r.c[i], acc)
        acc = np.where(acc > 1, F32(1.0), acc)
    if len(lights):
        r.k = np.where(active, acc, F32(1.0)).astype(F32)
    return r


class Combined:
    """refl: reflect_ref's Reflected (p, R, bounce, tri2, n2, kinds, ...).
    at_p / at_p2: shadow_at at the hit points (own object: the pixel's) and at
    the points the bounces meet (own object: the bounce's).  hit2: the bounce
    met something.  mask2: rt_shadow_hits_reflected's frame.  k, k2: the two
    shadowed factors.  lit: rt_light_hits_shadowed's int32x4 frame.
    mirrored(r): rt_light_hits_shadowed_reflected's."""

    def mirrored(self, r):
        return rr.blended(self.lit, r, self._lit, self._lit2, self.refl)


def shadow_reflect_ref(oracle, scene, hits, row_begin=0, ray_dir=REF_DIR, refl=None):
    """`refl`: reflect_ref's result for the same arguments, where the caller has it."""
    rf = refl if refl is not None else rr.reflect_ref(oracle, scene, hits, row_begin, ray_dir)
    t, obj = hits["t"], hits["object"]
    obj2, best = rf.bounce["object"], rf.bounce["t"]
    c = Combined()
    c.refl = rf
    c.hit2 = obj2 >= 0
    c.at_p = shadow_at(scene, obj.astype(np.int32),
                       (rf.surf["nx"], rf.surf["ny"], rf.surf["nz"]), rf.p)
    with np.errstate(all="ignore"):
        p2 = (rf.p[0] + best * rf.R[0], rf.p[1] + best * rf.R[1], rf.p[2] + best * rf.R[2])
    c.p2 = p2
    c.at_p2 = shadow_at(scene, obj2.astype(np.int32), rf.n2, p2)
    c.k, c.k2 = c.at_p.k, c.at_p2.k
    c.mask2 = np.where(c.hit2, c.at_p2.mask, np.uint32(0)).astype(np.uint32)
    c.lit = lr.lit_ref(oracle, scene, hits, row_begin, ray_dir, surf=rf.surf, k=c.k)
    with np.errstate(all="ignore"):
        c._lit = rr.ramp(t, False) * c.k
        c._lit2 = np.where(c.hit2, rr.ramp(t + best, True) * c.k2, F32(0.0)).astype(F32)
    return c


# ---------------------------------------------------------------------------
# What the tests of both files (CPU and GPU) share
# ---------------------------------------------------------------------------
def restated(oracle, key, scene, w, h, rows=None, d=REF_DIR):
    """(hits, shadow_reflect_ref's restatement), once per key, direction and
    light set, on top of reflect_ref.restated's for the same arguments."""
    _, rf = rr.restated(oracle, key, scene, w, h, rows, d)

    def shadow_reflect(oracle, scene, hits, row_begin, ray_dir):
        return shadow_reflect_ref(oracle, scene, hits, row_begin, ray_dir, refl=rf)
    return lr.restated(shadow_reflect, oracle, key, scene, w, h, rows, d)


def class_facts(scene, hits, c):
    """What the class scene is there for, each in at least one pixel (the
    restatement's counts stand beside the bounds)."""
    obj, obj2, nc = hits["object"], c.refl.bounce["object"], scene.num_cubes
    a, a2 = c.at_p, c.at_p2
    slot = np.arange(a2.by_object.shape[1])[None, :, None, None]
    by_own = (a2.by_object & (slot == obj[None, None])).any(1)
    by_third = (a2.by_object & (slot != obj[None, None])).any(1)
    assert not (a2.by_object & (slot == obj2[None, None])).any()  # obj2 is left out, always
    assert (by_third & ~by_own).any(0).sum() >= 100  # a third object alone hides the light: 365
    assert (by_own & ~by_third).any(0).sum() >= 50   # the pixel's own object alone: 190
    assert (a2.cast & ~a2.occluded).any(0).sum() >= 500  # an unoccluded facing light: 1268
    assert (c.hit2 & ~a2.cast.any(0)).sum() >= 20         # no facing light: 47
    assert a2.by_cube.any(0).sum() >= 30 and a2.by_sphere.any(0).sum() >= 100  # 78, 591
    shadowed, shadowed2 = a.occluded.any(0), a2.occluded.any(0)
    assert (shadowed2 & (obj2 < nc)).sum() >= 100 and (shadowed2 & (obj2 >= nc)).sum() >= 50
    assert (shadowed & c.hit2 & ~shadowed2).sum() >= 50   # at p, not at p2: 171
    assert (shadowed2 & ~shadowed).sum() >= 100           # at p2, not at p: 432
    # the primary object's shadow at p2 shows in the mask and in the colour
    own_only = (by_own & ~by_third).any(0)
    assert (c.mask2[own_only] != 0).all()
    assert (c.k2[own_only] < c.refl.k2[own_only]).all()


# the first light faces nothing the bounces meet; the second, below and beside
# the spheres, is seen from inside sphere 0 through sphere 0's own far side
INSIDE_LIGHTS = [(32, 24, 100, 1), (100, 24, -100, 1)]
SPECIAL_NAMES = ["twins", "sphere_tie", "ramp", "intersecting_spheres"]


def special_scenes(pkg):
    """name -> (scene, hit-cache key)."""
    return {
        "twins": (lr.with_lights(rr.twin_cubes_scene(pkg), lr.THREE_LIGHTS), "reflect_twins"),
        "sphere_tie": (lr.with_lights(rr.sphere_tie_scene(pkg), lr.THREE_LIGHTS),
                       "reflect_sphere_tie"),
        "ramp": (rr.ramp_scene(pkg, lr.THREE_LIGHTS), "reflect_ramp"),
        "intersecting_spheres": (sr.intersecting_spheres(pkg, [(32, 24, 100, 1), (32, 24, 0, 1)]),
                                 "shadow_edge_p_inside_a_sphere"),
    }
