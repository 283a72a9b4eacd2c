"""rt_shadow_hits / rt_light_hits_shadowed without a GPU: the host functions
against the numpy restatement (tests/shadow_ref.py) of DESIGN.md §3.1b.

Every comparison is on raw 32-bit words; there are no tolerances.  Every case
first asserts on the restatement that it contains what it is there for.
"""
import shutil

import numpy as np
import pytest

import light_contract as lc
import light_ref as lr
import shadow_ref as sr
from gpu_support import H, W
from hit_ref import K_FAR, REF_DIR
from light_ref import ONE_LIGHT, THREE_LIGHTS, base, eq, one_cube, one_sphere

ENTRIES = lc.ENTRIES["shadow"]
F32 = np.float32
BLACK = (0, 0, 0, 255)


def compare(pkg, oracle, scene, hits, rows=None, d=REF_DIR, label="", mask=True):
    """Mask and both lit formats of the host functions against the
    restatement; returns the restatement."""
    r = sr.shadow_ref(oracle, scene, hits, rows[0] if rows else 0, d)
    if mask:
        got = pkg.shadow_hits(hits, scene, rows=rows, ray_dir=d)
        assert got.dtype == np.uint32 and got.shape == hits.shape
        assert np.array_equal(got, r.mask), f"{label} mask: {eq(got, r.mask)}"
    for fmt, ref in (("i32x4", r.lit), ("rgba8", oracle.pack_rgba8(r.lit))):
        got = pkg.light_hits(hits, scene, fmt, rows=rows, ray_dir=d, shadows=True)
        assert got.dtype == ref.dtype and not eq(got, ref), f"{label} {fmt}: {eq(got, ref)}"
    return r


# --- 1. the four occluder / receiver kinds -----------------------------------------
def test_the_four_kinds(pkg, oracle):
    scene = sr.kinds_scene(pkg)
    w, h = sr.KINDS_W, sr.KINDS_H
    hits = lr.cached_hits(oracle, "shadow_kinds", scene, w, h)
    obj = hits["object"]
    assert set(np.unique(obj).tolist()) == {0, 1, 2}  # sphere 1 (slot 3) is never seen
    r = compare(pkg, oracle, scene, hits, label="kinds")
    cube, sphere = obj < 2, obj == 2
    # the restatement's counts: 1076 cube -> cube, 1168 sphere 0 -> the face and
    # 102 sphere 1 -> the box, 271 cube -> sphere, 168 sphere -> sphere; 1619
    # shadowed pixels in all, 50 mixed 64-pixel row segments
    assert (r.by_cube[0] & cube).sum() >= 50
    assert (r.by_sphere[0] & (obj == 0)).sum() >= 50 and (r.by_sphere[0] & (obj == 1)).sum() >= 50
    assert (r.by_cube[0] & sphere).sum() >= 50
    assert (r.by_sphere[0] & sphere).sum() >= 50
    assert sr.segments(r.mask != 0)[2] >= 10
    assert set(np.unique(r.mask).tolist()) == {0, 1}
    # shadowed != unshadowed exactly where a blocked light's c is nonzero after
    # rounding, i.e. where it gave the unshadowed pixel a nonzero channel
    shadowed, unshadowed = pkg.light_hits(hits, scene, shadows=True), pkg.light_hits(hits, scene)
    changed = (r.mask != 0) & (unshadowed[..., :3] != 0).any(-1)
    assert changed.sum() > 1000
    assert np.array_equal((shadowed != unshadowed).any(-1), changed)
    dark = (r.k == 0) & (obj >= 0)
    assert (dark & (r.mask != 0)).sum() > 1000 and (hits["t"][dark] != K_FAR).all()
    assert (shadowed[dark] == BLACK).all()
    assert (pkg.light_hits(hits, scene, "rgba8", shadows=True)[dark] == 0xFF000000).all()


# --- 2. the hit object is never an occluder ------------------------------------------
def apart(pkg):
    """Two spheres side by side and a light in front of the gap: no segment
    from one of them to the light comes near the other."""
    return pkg.Scene(np.array([[16, 24, -50, 1], [48, 24, -50, 1]], F32), np.array([10, 10], F32),
                     np.array([[1, 0.5, 0.25, 255], [0.25, 0.5, 1, 255]], F32))


SELF_SCENES = {
    "cube": lambda pkg: one_cube(pkg, [("scale", 15, 15, 10), ("translate", 32, 24, -50)],
                                 (1, 1, 1, 255)),
    "rotated_cube": lambda pkg: one_cube(pkg, [("scale", 12, 12, 12), ("rotate", .3, .7, .1),
                                               ("translate", 32, 24, -40)], (1, 0.5, 0.25, 255)),
    "sphere": lambda pkg: one_sphere(pkg, (32, 24, -50, 1), 20, (1.0, 0.5, 0.25, 255)),
    "two_spheres_apart": apart,
}


@pytest.mark.parametrize("name", sorted(SELF_SCENES))
def test_self_exclusion(pkg, oracle, name):
    lights = [(32, 24, 100, 1)] if name == "two_spheres_apart" else THREE_LIGHTS
    scene = lr.with_lights(SELF_SCENES[name](pkg), lights)
    w, h = 64, 48
    hits = lr.cached_hits(oracle, "shadow_self_" + name, scene, w, h)
    r = compare(pkg, oracle, scene, hits, label=name)
    assert r.cast.any(1).any(1).all() and r.cast.sum() > 300  # every light casts rays
    if name == "two_spheres_apart":
        assert ((hits["object"] == 0) & r.cast[0]).sum() > 100
        assert ((hits["object"] == 1) & r.cast[0]).sum() > 100
    assert not r.mask.any()
    assert not pkg.shadow_hits(hits, scene).any()
    for fmt in ("i32x4", "rgba8"):
        a, b = pkg.light_hits(hits, scene, fmt, shadows=True), pkg.light_hits(hits, scene, fmt)
        assert not eq(a, b), f"{name} {fmt}: {eq(a, b)}"


# --- 3. the base scene -----------------------------------------------------------------
@pytest.mark.parametrize("lights", [[], ONE_LIGHT, THREE_LIGHTS], ids=["0", "1", "3"])
@pytest.mark.parametrize("key,w,h,rows", [("96x80", W, H, None), ("83x45_rows_7_38", 83, 45, (7, 38))],
                         ids=["96x80", "83x45_rows_7_38"])
def test_base_scene(pkg, oracle, key, w, h, rows, lights):
    scene = lr.with_lights(base(pkg), lights)
    hits = lr.cached_hits(oracle, "base", scene, w, h, rows, REF_DIR)
    r = compare(pkg, oracle, scene, hits, rows=rows, label=key)
    if not lights:
        assert not r.mask.any()
        for fmt in ("i32x4", "rgba8"):
            a = pkg.light_hits(hits, scene, fmt, rows=rows, shadows=True)
            assert not eq(a, pkg.shade_hits(hits, scene, fmt))
    else:
        assert (r.mask != 0).sum() > 20 and r.by_cube.sum() > 0 and r.by_sphere.sum() > 20
        assert ((r.mask == 0) & r.cast.any(0)).sum() > 100  # and lit pixels that see a light


# --- 4. bits are per light ---------------------------------------------------------------
PER_LIGHT = [sr.KINDS_LIGHT, (64, 64, 300, 1), (-26, 64, 40, 1)]


def test_bits_are_per_light(pkg, oracle):
    scene = sr.kinds_scene(pkg, PER_LIGHT)
    hits = lr.cached_hits(oracle, "shadow_kinds", scene, sr.KINDS_W, sr.KINDS_H)
    r = compare(pkg, oracle, scene, hits, label="per light")
    assert (r.mask == 1).sum() > 50 and (r.mask == 4).sum() > 50  # the first only, the third only
    assert r.cast.all(0).sum() > 10000


def test_33_lights(pkg, oracle):
    """The mask has 32 bits: refused.  The lit frame has no such limit."""
    lights = PER_LIGHT + [(10 + 4 * i, 20 + 3 * i, 30 + i, 1) for i in range(30)]
    scene = sr.kinds_scene(pkg, lights)
    assert len(scene.lights) == 33
    hits = lr.cached_hits(oracle, "shadow_kinds", scene, sr.KINDS_W, sr.KINDS_H)
    lc.more_than_32_lights(pkg, ENTRIES, scene, hits)
    r = compare(pkg, oracle, scene, hits, label="33 lights", mask=False)
    assert r.occluded[32].sum() > 50 and r.cast[32].sum() > 1000


# --- 5. numeric edges ----------------------------------------------------------------------
def check_edge(name, scene, hits, r):
    """The restatement holds what the case is there for."""
    obj, t = hits["object"], hits["t"]
    if name == "light_on_a_hit_point":
        assert obj[40, 40] == 0 and t[40, 40] == 50 and np.isnan(r.c[0][40, 40])
        assert not r.cast[0][obj == 0].any()  # L lies in the face's plane: c = 0
        assert r.occluded[1].sum() > 1000
    elif name == "light_at_1e20":
        # at 1e20 ll is infinite and c = 0: no ray; at 1e19 a is finite, b * b and
        # a * q are not, disc = inf - inf: no sphere occludes, the fp64 cubes still do
        assert not r.cast[0].any() and not r.cast[1].any() and r.cast[2].sum() > 10000
        assert not r.by_sphere[2].any() and r.by_cube[2].sum() > 50
    elif name == "light_at_inf":
        assert np.isnan(r.c).any() and not r.mask.any()
    elif name == "light_at_nan":
        assert not r.cast[0].any() and not r.cast[2].any() and r.occluded[1].sum() > 1000
    elif name == "light_at_denormals":
        assert r.cast[0].sum() > 10000 and r.occluded[1].sum() > 1000
    elif name == "light_inside_a_sphere":
        face = obj == 0
        assert (r.by_sphere[0] & face).sum() > 10000  # the whole face but what the box hides
        assert not r.cast[0][obj > 0].any()  # its own sphere and the box face away
    elif name == "light_on_a_triangle":
        p = lr.hit_points(hits, 0, REF_DIR)
        L = tuple(F32(v) - a for v, a in zip((91, 64, -15), p))
        back = [k for k in range(12)
                if (scene.cube_vertices[1, 3 * k:3 * k + 3, 2] == -15).all()]
        assert len(back) == 2
        at_light = np.zeros(hits.shape, bool)
        for k in back:
            ok, td = sr.tri_td(p, L, *scene.cube_vertices[1, 3 * k:3 * k + 3])
            at_light |= ok & (td == 1.0) & (obj == 0)
        assert at_light.sum() > 50  # t == 1.0 exactly: not occluding
        assert not (r.by_cube[0] & at_light).any()
    elif name == "p_inside_a_sphere":
        on = obj == 1
        assert on.sum() > 100 and (obj[obj >= 0] == 1).all()
        c, rad = scene.sphere_origins[0], scene.sphere_radius[0]
        p = lr.hit_points(hits, 0, REF_DIR)
        inside = ((p[0] - c[0]) ** 2 + (p[1] - c[1]) ** 2 + (p[2] - c[2]) ** 2) < rad * rad
        assert (inside & on & r.cast[0]).sum() > 50
        assert (r.occluded[0] & inside).sum() > 50      # the light outside: s1 in (0, 1)
        assert not (r.occluded[1] & inside).any() and (r.cast[1] & inside).sum() > 50
    elif name == "minus_inf":
        assert np.isneginf(t).sum() > 50 and not r.cast.any()
    elif name == "nan_colour":
        assert np.isnan(scene.sphere_colours).any() and r.cast.sum() > 50 and not r.mask.any()
    else:
        raise AssertionError(name)


EDGE_NAMES = sorted(sr.EDGE_LIGHTS) + ["p_inside_a_sphere", "minus_inf", "nan_colour"]


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_numeric_edges(pkg, oracle, name):
    cases = {c[0]: c for c in sr.edge_cases(pkg)}
    assert sorted(cases) == sorted(EDGE_NAMES)
    _, scene, w, h, d = cases[name]
    key = "shadow_kinds" if name in sr.EDGE_LIGHTS else "shadow_edge_" + name
    hits = lr.cached_hits(oracle, key, scene, w, h, None, d)
    r = compare(pkg, oracle, scene, hits, d=d, label=name)
    check_edge(name, scene, hits, r)


# --- 6. the argument contract ------------------------------------------------------------------
def test_object_out_of_range_is_refused(pkg):
    lc.objects_out_of_range(pkg, ENTRIES)


def test_formats_widths_and_rows_are_refused(pkg):
    lc.formats_widths_rows_and_pointers(pkg, ENTRIES)


def test_device_entries_refuse_a_null_context(pkg):
    """Before any HIP call: this runs without a GPU."""
    lc.device_entries_refuse_bad_arguments(pkg, ENTRIES)


def test_python_mirror_names(pkg):
    lc.names(pkg, ENTRIES)


# --- 7. under the sanitizers ------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shadow_arguments_under_sanitizers(tmp_path):
    """tests/shadow_args_check.cpp: exactly-sized heap arrays, the four-kinds
    scene, an empty scene with NULL arrays, a band, 33 lights."""
    lc.run_args_check(tmp_path, "shadow")
