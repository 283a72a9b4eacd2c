"""rt_reflect_hits / rt_light_hits_reflected without a GPU: the host functions
against the numpy restatement (tests/reflect_ref.py) of DESIGN.md §3.1c.

Every comparison is on raw 32-bit words; there are no tolerances and no words
are masked.  Every case first asserts on the restatement that it contains what
it is there for.

A NaN that an operation creates has no specified sign (§3.1a).  None can reach
an output word here: `best` is only ever written from a value that passed
`sf < best`, which NaN fails, and a lit channel goes through (int), which
turns every NaN into INT32_MIN.  `test_no_nan_reaches_a_bounce_frame` checks
the first on the restatement.
"""
import shutil

import numpy as np
import pytest

import light_contract as lc
import light_ref as lr
import reflect_ref as rr
import shadow_ref as sr
from gpu_support import H, W
from hit_ref import K_FAR, REF_DIR
from light_ref import ONE_LIGHT, THREE_LIGHTS, base, eq, one_cube, one_sphere

F32 = np.float32
REFLECTIVITIES = (0.25, 1.0)
ENTRIES = lc.ENTRIES["reflect"]
restated = rr.restated


def compare(pkg, oracle, scene, hits, r, rows=None, d=REF_DIR, label=""):
    """The bounce frame and both lit formats, at r = 0, 0.25 and 1, of the
    host functions against the restatement `r`."""
    got = pkg.reflect_hits(hits, scene, rows=rows, ray_dir=d)
    assert got.dtype == pkg.HIT_DTYPE and got.shape == hits.shape
    assert not eq(got, r.bounce), f"{label} bounce: {eq(got, r.bounce)}"
    for refl in (0.0,) + REFLECTIVITIES:
        want = r.mirrored(refl)
        for fmt, ref in (("i32x4", want), ("rgba8", oracle.pack_rgba8(want))):
            got = pkg.light_hits_reflected(hits, scene, refl, fmt, rows=rows, ray_dir=d)
            assert got.dtype == ref.dtype and not eq(got, ref), \
                f"{label} r={refl} {fmt}: {eq(got, ref)}"


# --- 1. the four receiver / target kinds -------------------------------------------------
def test_the_four_kinds(pkg, oracle):
    scene = rr.mirror_scene(pkg)
    hits, r = restated(oracle, "mirror", scene, rr.MIRROR_W, rr.MIRROR_H)
    for kind, frame in r.kinds.items():  # the restatement: 210, 400, 500 and 248 pixels
        assert frame.sum() >= 100, kind
    assert ((hits["object"] >= 0) & (r.bounce["object"] == -1)).sum() >= 1000  # bounce misses
    assert (r.bounce["t"][r.bounce["object"] == -1] == K_FAR).all()
    compare(pkg, oracle, scene, hits, r, label="kinds")
    # a mirrored pixel differs from the unmirrored one, and r = 1 shows the target alone
    mirrored = r.bounce["object"] >= 0
    full, plain = pkg.light_hits_reflected(hits, scene, 1.0), pkg.light_hits(hits, scene)
    assert ((full != plain).any(-1) & mirrored).sum() >= 500
    assert (full[(hits["object"] >= 0) & ~mirrored] == (0, 0, 0, 255)).all()


def test_factor_at_is_light_factor(pkg, oracle):
    """reflect_ref.factor_at (k2) against light_ref.light_factor_ref on the
    primary pixels: one text for both."""
    scene = rr.mirror_scene(pkg)
    hits, r = restated(oracle, "mirror", scene, rr.MIRROR_W, rr.MIRROR_H)
    k = rr.factor_at((r.surf["nx"], r.surf["ny"], r.surf["nz"]), r.p, scene.lights)
    assert ((r.k > 0) & (r.k < 1)).sum() > 1000
    assert np.array_equal(k.view(np.uint32), r.k.view(np.uint32))


def test_an_object_no_primary_ray_sees(pkg, oracle):
    scene = rr.mirror_scene(pkg)
    hits, r = restated(oracle, "mirror", scene, rr.MIRROR_W, rr.MIRROR_H)
    slot = scene.num_cubes + 1  # sphere 1 of kinds_scene
    assert not (hits["object"] == slot).any()
    assert (r.bounce["object"] == slot).sum() >= 20
    got = pkg.reflect_hits(hits, scene)
    assert np.array_equal(got["object"] == slot, r.bounce["object"] == slot)
    # straight back from the face at z = -50 to a sphere that ends at z = 8
    assert (got["t"][got["object"] == slot] >= 58).all()


# --- 2. the hit object is never a candidate ---------------------------------------------
SELF_SCENES = {
    "cube": lambda pkg: one_cube(pkg, [("scale", 15, 15, 10), ("translate", 32, 24, -50)],
                                 (1, 1, 1, 255)),
    "sphere": lambda pkg: one_sphere(pkg, (32, 24, -50, 1), 20, (1.0, 0.5, 0.25, 255)),
}


@pytest.mark.parametrize("name", sorted(SELF_SCENES))
def test_self_exclusion(pkg, oracle, name):
    scene = lr.with_lights(SELF_SCENES[name](pkg), THREE_LIGHTS)
    hits, r = restated(oracle, "reflect_self_" + name, scene, 64, 48)
    assert (hits["object"] == 0).sum() > 500
    compare(pkg, oracle, scene, hits, r, label=name)
    got = pkg.reflect_hits(hits, scene)
    assert (got["object"] == -1).all() and (got["t"] == K_FAR).all()
    # every channel is (int)(a + r * (0 - a))
    on = hits["object"] == 0
    for refl in REFLECTIVITIES:
        lit = pkg.light_hits_reflected(hits, scene, refl)
        for ch in range(3):
            a = r._lit * r._colour[..., ch]
            want = lr.x86_int(a + F32(refl) * (F32(0.0) - a))
            assert np.array_equal(lit[..., ch][on], want[on]), (name, refl, ch)
        assert (lit[~on] == (0, 0, 0, 255)).all()
    assert (pkg.light_hits_reflected(hits, scene, 1.0)[..., :3] == 0).all()


# --- 3. ties go to the first candidate ---------------------------------------------------
def test_identical_cubes_give_the_lower_slot(pkg, oracle):
    scene = rr.twin_cubes_scene(pkg)
    assert np.array_equal(scene.cube_vertices[0], scene.cube_vertices[1])
    hits, r = restated(oracle, "reflect_twins", scene, 64, 48)
    sphere = hits["object"] == 2
    assert (sphere & (r.bounce["object"] == 0)).sum() >= 20  # the restatement: 26
    assert not (r.bounce["object"] == 1).any()
    compare(pkg, oracle, scene, hits, r, label="twins")


def test_a_sphere_and_a_triangle_at_one_distance_give_the_cube(pkg, oracle):
    scene = rr.sphere_tie_scene(pkg)
    hits, r = restated(oracle, "reflect_sphere_tie", scene, 64, 48)
    y, x = rr.TIE_PIXEL
    assert hits["object"][y, x] == 1
    p = tuple(a[y:y + 1, x:x + 1] for a in r.p)
    R = tuple(a[y:y + 1, x:x + 1] for a in r.R)
    tri = [rr.tri_sf(p, R, *scene.cube_vertices[0, 3 * k:3 * k + 3]) for k in range(12)]
    tri = [sf[0, 0] for ok, sf in tri if ok[0, 0]]
    ok, s0, far = rr.sphere_sf(p, R, scene.sphere_origins[0], scene.sphere_radius[0])
    assert ok[0, 0] and not far[0, 0] and len(tri) >= 1
    assert min(tri).view(np.uint32) == s0[0, 0].view(np.uint32)  # equal as floats
    assert r.bounce["object"][y, x] == 0 and r.bounce["t"][y, x] == s0[0, 0]
    assert (r.bounce["object"] == 2).sum() >= 50  # and the sphere wins where it is nearer
    compare(pkg, oracle, scene, hits, r, label="sphere tie")
    assert pkg.reflect_hits(hits, scene)["object"][y, x] == 0


# --- 4. a hit point inside another sphere ---------------------------------------------------
def test_hit_point_inside_another_sphere(pkg, oracle):
    scene = sr.intersecting_spheres(pkg, [(32, 24, 100, 1)])
    hits, r = restated(oracle, "shadow_edge_p_inside_a_sphere", scene, 64, 48)
    on = hits["object"] == 1
    assert on.sum() > 100 and (hits["object"][hits["object"] >= 0] == 1).all()
    c, rad = scene.sphere_origins[0], scene.sphere_radius[0]
    inside = ((r.p[0] - c[0]) ** 2 + (r.p[1] - c[1]) ** 2 + (r.p[2] - c[2]) ** 2) < rad * rad
    took_s1 = r.far_root & (r.bounce["object"] == 0)
    assert (took_s1 & inside & on).sum() > 100  # the restatement: 193
    compare(pkg, oracle, scene, hits, r, label="inside a sphere")


# --- 5. reflectivity 0 is rt_light_hits -------------------------------------------------------
def zero_cases(pkg):
    cases = [(f"base_{len(l)}", lr.with_lights(base(pkg), l), W, H, REF_DIR, "base")
             for l in ([], ONE_LIGHT, THREE_LIGHTS)]
    for key, scene, w, h, d in lr.edge_scenes(pkg):
        if key in ("minus_inf", "nan_colour"):
            cases.append((key, lr.with_lights(scene, THREE_LIGHTS), w, h, d, "shadow_edge_" + key))
    return {c[0]: c for c in cases}


@pytest.mark.parametrize("name", ["base_0", "base_1", "base_3", "minus_inf", "nan_colour"])
def test_reflectivity_zero(pkg, oracle, name):
    _, scene, w, h, d, key = zero_cases(pkg)[name]
    hits = lr.cached_hits(oracle, key, scene, w, h, None, d)
    assert (hits["object"] >= 0).sum() > 100
    if name == "minus_inf":
        assert np.isneginf(hits["t"]).sum() > 50
    if name == "nan_colour":
        assert np.isnan(scene.sphere_colours).any()
    for refl in (0.0, -0.0):
        for fmt in ("i32x4", "rgba8"):
            got = pkg.light_hits_reflected(hits, scene, refl, fmt, ray_dir=d)
            want = pkg.light_hits(hits, scene, fmt, ray_dir=d)
            assert got.dtype == want.dtype and not eq(got, want), f"{name} {fmt}: {eq(got, want)}"
    if name.startswith("base"):
        _, r = restated(oracle, key, scene, w, h, None, d)
        assert (r.bounce["object"] >= 0).sum() > 300  # r = 0.25 would have changed them
        assert eq(pkg.light_hits_reflected(hits, scene, 0.25), pkg.light_hits(hits, scene))


@pytest.mark.parametrize("lights", [[], ONE_LIGHT, THREE_LIGHTS], ids=["0", "1", "3"])
def test_base_scene(pkg, oracle, lights):
    scene = lr.with_lights(base(pkg), lights)
    hits, r = restated(oracle, "base", scene, W, H)
    assert min(v.sum() for v in r.kinds.values()) >= 50  # the restatement: 59, 114, 185, 283
    if lights:
        assert ((r.k2 > 0) & (r.k2 < 1)).sum() > 100
    compare(pkg, oracle, scene, hits, r, label="base")


# --- 6. the ramp's end ---------------------------------------------------------------------------
@pytest.mark.parametrize("lights", [[], ONE_LIGHT], ids=["0", "1"])
def test_beyond_the_ramps_end(pkg, oracle, lights):
    """t + best > 180: the bounce adds 0, not negative light."""
    scene = rr.ramp_scene(pkg, lights)
    hits, r = restated(oracle, "reflect_ramp", scene, 64, 48)
    past = (hits["t"] + r.bounce["t"] > 180) & (r.bounce["object"] == 1)
    assert past.sum() >= 200 and (r.scalar2[past] < 0).all()  # the restatement: 317
    compare(pkg, oracle, scene, hits, r, label="ramp")
    full = pkg.light_hits_reflected(hits, scene, 1.0)
    assert (full[past] == (0, 0, 0, 255)).all()
    quarter = pkg.light_hits_reflected(hits, scene, 0.25)
    assert (quarter[past][:, :3] >= 0).all() and (quarter[past][:, 0] > 0).all()


# --- 7. numeric edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rr.EDGE_NAMES)
def test_numeric_edges(pkg, oracle, name):
    cases = rr.edge_cases(pkg)
    assert sorted(cases) == sorted(rr.EDGE_NAMES)
    scene, w, h, d, key = cases[name]
    hits, r = restated(oracle, key, scene, w, h, None, d)
    rr.check_edge(name, scene, hits, r)
    compare(pkg, oracle, scene, hits, r, d=d, label=name)


def test_no_nan_reaches_a_bounce_frame(pkg, oracle):
    """Over every edge case: `best` is a number everywhere (a NaN candidate
    fails sf < best), so no output word of a bounce frame is a created NaN."""
    for name, (scene, w, h, d, key) in rr.edge_cases(pkg).items():
        _, r = restated(oracle, key, scene, w, h, None, d)
        assert not np.isnan(r.bounce["t"]).any(), name
        assert (r.bounce["t"] <= K_FAR).all(), name


# --- 8. bands --------------------------------------------------------------------------------------
def test_a_band_is_a_slice_of_the_frame(pkg, oracle):
    scene = rr.mirror_scene(pkg)
    w, h, rows = rr.MIRROR_W, rr.MIRROR_H, (21, 109)
    hits, r = restated(oracle, "mirror", scene, w, h)
    band = np.ascontiguousarray(hits[rows[0]:rows[1]])
    assert (r.bounce["object"][rows[0]:rows[1]] >= 0).sum() >= 1000
    got = pkg.reflect_hits(band, scene, rows=rows)
    assert not eq(got, r.bounce[rows[0]:rows[1]])
    for fmt in ("i32x4", "rgba8"):
        whole = pkg.light_hits_reflected(hits, scene, 0.25, fmt)
        got = pkg.light_hits_reflected(band, scene, 0.25, fmt, rows=rows)
        assert not eq(got, whole[rows[0]:rows[1]]), fmt
    # the same band taken for rows 0..88 is another picture
    assert eq(pkg.reflect_hits(band, scene), r.bounce[rows[0]:rows[1]])


# --- 9. the argument contract ---------------------------------------------------------------------
def test_object_out_of_range_is_refused(pkg):
    lc.objects_out_of_range(pkg, ENTRIES)


def test_reflectivity_outside_0_1_is_refused(pkg):
    scene = base(pkg)
    hits = np.zeros((2, 3), pkg.HIT_DTYPE)
    hits["t"], hits["object"] = K_FAR, -1
    for refl in (0.0, 1.0, 0.5, float(np.nextafter(F32(1), F32(0)))):
        assert pkg.light_hits_reflected(hits, scene, refl).shape == (2, 3, 4)
    for refl in (-0.1, 1.5, float("nan"), float(np.nextafter(F32(1), F32(2))), -1e-30,
                 float("inf")):
        for fmt in ("i32x4", "rgba8"):
            lc.refused(pkg, lambda: pkg.light_hits_reflected(hits, scene, refl, fmt))


def test_formats_widths_rows_and_pointers_are_refused(pkg):
    lc.formats_widths_rows_and_pointers(pkg, ENTRIES)


def test_device_entries_refuse_bad_arguments_before_any_hip_call(pkg):
    lc.device_entries_refuse_bad_arguments(pkg, ENTRIES)


def test_python_mirror_names(pkg):
    lc.names(pkg, ENTRIES)
    lc.names(pkg, lc.ENTRIES["light"])  # light_hits and light_hits_device keep their signatures


# --- 10. under the sanitizers ----------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_reflect_arguments_under_sanitizers(tmp_path):
    """tests/reflect_args_check.cpp: exactly-sized heap arrays, a scene of all
    four kinds, an empty scene with NULL arrays, a band, the refusals."""
    lc.run_args_check(tmp_path, "reflect")
